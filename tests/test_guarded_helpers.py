"""CPU self-tests of tests/guarded.py: each check must trip on the defect it exists for (simulated kernels writing into a
device='cpu' guarded buffer) and stay quiet on a correct write."""
import pytest
import torch

from common import relerr
from guarded import LOCAL_TOL, guard_bytes, guarded_in, guarded_out, tile_err


def _kernel(g, src, rows=None, extra=0):
    """A 'kernel' that stores `src` row by row into the guarded output through its raw byte address, the way a HIP kernel
    sees it: `rows` limits the rows stored (a skipped tile), `extra` elements are stored past the logical end."""
    flat = src.reshape(-1)
    es = flat.element_size()
    raw = g.buf[g.guard:g.guard + (flat.numel() + extra) * es].view(src.dtype)
    cols = src.shape[-1]
    for r in (range(src.shape[0]) if rows is None else rows):
        raw[r * cols:(r + 1) * cols] = flat[r * cols:(r + 1) * cols]
    if extra:
        raw[flat.numel():] = flat[-extra:]


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_correct_write_passes(dtype):
    src = torch.randn(100, 40).to(dtype)
    g = guarded_out(src.shape, dtype, device='cpu')
    _kernel(g, src)
    assert torch.equal(g.check(), src)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_one_element_past_the_end_trips_check_guards(dtype):
    src = torch.randn(100, 40).to(dtype)
    g = guarded_out(src.shape, dtype, device='cpu')
    _kernel(g, src, extra=1)
    g.assert_written()                         # the logical output itself is complete ...
    with pytest.raises(AssertionError, match='back guard damaged'):
        g.check_guards()                       # ... but one element landed behind it


def test_store_before_the_start_trips_check_guards():
    g = guarded_out((64, 32), torch.float16, device='cpu')
    g.buf[g.guard - 2:g.guard].view(torch.float16)[0] = 1.0
    with pytest.raises(AssertionError, match='front guard damaged'):
        g.check_guards()


def test_skipped_32_row_tile_trips_assert_written():
    src = torch.randn(200, 64).half()
    g = guarded_out(src.shape, torch.float16, device='cpu')
    _kernel(g, src, rows=[r for r in range(200) if not 64 <= r < 96])
    g.check_guards()
    with pytest.raises(AssertionError, match='never written'):
        g.assert_written()
    g.assert_written((slice(0, 64),))          # a region check sees only its own rows


def test_untouched_region():
    g = guarded_out((2, 8, 64), torch.float16, device='cpu')
    g.t[:, :, :50] = 1.0
    g.check((slice(None), slice(None), slice(0, 50)))
    g.assert_untouched((slice(None), slice(None), slice(50, None)))
    g.t[1, 3, 50] = 0.0
    with pytest.raises(AssertionError, match='outside the logical output'):
        g.assert_untouched((slice(None), slice(None), slice(50, None)))


def test_uint8_needs_two_fills():
    src = torch.randint(0, 256, (64, 48), dtype=torch.uint8)
    src[5, 7], src[6, 8] = 0, 255
    outs = []
    for fill in (0x00, 0xFF):
        g = guarded_out(src.shape, torch.uint8, device='cpu', fill=fill)
        _kernel(g, src, rows=[r for r in range(64) if r != 5])        # row 5 skipped: invisible to one fill alone
        g.check_guards()
        outs.append(g.t.clone())
    assert not torch.equal(outs[0], outs[1])


def test_non_finite_output_trips_check():
    src = torch.randn(64, 32).half()
    src[3, 4] = float('inf')
    g = guarded_out(src.shape, torch.float16, device='cpu')
    _kernel(g, src)
    with pytest.raises(AssertionError, match='non-finite'):
        g.check()


def test_ragged_last_tile_1pct_off_trips_tile_err_but_not_relerr():
    M, N = 66000, 16
    ref = torch.randn(M, N, dtype=torch.float64)
    got = ref.clone()
    got[-208:] *= 1.01                          # the ragged last row tile of M = 66000 on 256-row tiles
    assert relerr(got, ref) < 1e-3             # the normwise error does not see it ...
    assert tile_err(got, ref, (32, 32)) > LOCAL_TOL        # ... the blockwise one does
    assert tile_err(ref.half().float(), ref, (32, 32)) < LOCAL_TOL / 4      # fp16 storage alone: well inside the bound


def test_one_wrong_block_trips_tile_err():
    ref = torch.randn(4096, 1280)
    got = ref.clone()
    got[1024:1056, 640:672] *= 1.05                 # one 32 x 32 block 5 % off
    assert relerr(got, ref) < 1e-3
    assert tile_err(got, ref, (32, 32)) > LOCAL_TOL


def test_tile_err_floor_on_near_zero_blocks():
    ref = torch.randn(256, 64)
    ref[:32, :32] = 1e-6                        # a block of (almost) zeros: judged against 0.25 rms, not against itself
    got = ref.clone()
    got[:32, :32] = 1e-6 + 1e-5
    assert tile_err(got, ref, (32, 32)) < LOCAL_TOL


def test_guarded_in_reads_past_the_end_are_nan():
    x = torch.randn(10, 64).half()
    d = guarded_in(x, device='cpu')
    assert torch.equal(d, x)
    base = d.data_ptr()
    g = guard_bytes(x.shape, x.dtype)
    storage = torch.empty(0, dtype=torch.float16).set_(d.untyped_storage(), 0, (d.untyped_storage().nbytes() // 2,))
    off = (base - storage.data_ptr()) // 2
    assert off * 2 == g
    assert bool(storage[off + x.numel():].isnan().all()) and bool(storage[:off].isnan().all())


def test_guard_size_and_alignment():
    assert guard_bytes((10, 4), torch.float16) == 64 * 1024
    assert guard_bytes((10, 1280), torch.float16) == 256 * 1280 * 2
    assert guard_bytes((1310720,), torch.float16) == 64 * 1024          # a flat output's row is one element
    assert guard_bytes((3, 77), torch.float16) % 256 == 0
    assert guard_bytes((3, 1001), torch.float32) % 256 == 0 and guard_bytes((3, 1001), torch.float32) >= 256 * 1001 * 4
