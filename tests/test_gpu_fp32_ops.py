"""Per-kernel parity for the fp32-side kernels of the text encoder and of the first stage, which were only ever judged through a
whole network (test_gpu_clip.py, test_gpu_vae.py, test_gpu_vae_encoder.py: 1.09 x floor of a whole tensor, O(1) hidden states,
prompts of [2, 77] or [5, 77]):

  k_embed_tokens                       fgdm_op_embed_tokens       exact
  k_add_f16_to_f32                     fgdm_op_add_f16_to_f32     exact
  k_f32_to_f16                         fgdm_op_f32_to_f16         exact
  k_silu_f32_to_f16                    fgdm_op_silu_f32_to_f16    one fp16 ulp of the float64 value
  ln32_kernel<half_t>, <float>         fgdm_op_layernorm32        bound derived from the kernel's operation order
  k_vae_prequant                       fgdm_op_vae_prequant       likewise, and exact on a permutation weight
  k_vae_moments                        fgdm_op_vae_moments        likewise, and exact on a permutation weight

Exact cases compare bits.  Bounded cases compare with float64 on the same fp32 inputs, element by element, against a bound that
follows from the kernel's own sequence of roundings (u = 2^-24, the fp32 unit roundoff); the worst err / bound of every case is
printed through common.report and must stay below 1.  No bound here was fitted to what the kernels return.

The sizes are the smallest that reach every path: n = 2^20 + 773 (elementwise), rows W / 4 = 1 049 664 (embedding) and
B HW = 1 048 839 (first stage) exceed the 4096 x 256 threads the launchers cap the grid at, so the grid-stride loop takes a second,
ragged trip; C = 252 and 1284 end ln32_kernel's 256-wide lane walk on a partial trip, C = 4 leaves 63 lanes idle, rows = 1 and 5
leave waves of the last block idle.

Every output sits in a guarded, poisoned buffer and every floating-point input between NaN guards (tests/guarded.py); every input
is drawn on the CPU from a seeded generator."""
import functools
import math

import pytest
import torch

from common import report
from guarded import guarded_out
from test_gpu_narrow_ops import ulp16
from test_gpu_ops import _p, _st, din, rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # fp32 unit roundoff
GRID_THREADS = 4096 * 256           # ew_grid / embed_tokens: at most 4096 blocks of 256 threads
EW_SIZES = (1, 255, 12345, GRID_THREADS + 773)


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def uniform(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=g)


def with_specials(x, specials):
    """x with `specials` at its front and, where it is long enough, at its very end as well (the last trip of the grid-stride loop)"""
    s = torch.tensor(specials, dtype=x.dtype)
    k = min(x.numel(), s.numel())
    x[:k] = s[:k]
    if x.numel() >= 2 * s.numel():
        x[-s.numel():] = s
    return x


def worst(what, err, bound):
    """the largest err / bound, reported; every element must satisfy err <= bound"""
    err, bound = err.reshape(-1), bound.expand(err.shape).reshape(-1)
    ratio = err / bound
    i = int(ratio.argmax())
    r = float(ratio[i])
    report(f'{what}: worst err / bound (|err| {float(err[i]):.3e}, bound {float(bound[i]):.3e})', r, 1.0)
    assert bool((err <= bound).all()), (what, r)
    return r


# ================================================================================================== elementwise, exact
def _below(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(0.0)))


def _above(v):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(math.copysign(math.inf, v))))


def convert_specials():
    """fp32 values at which a conversion to fp16 that is not round-to-nearest-even, or that flushes subnormals, shows"""
    t = 2.0 ** -24                                          # the fp16 subnormal spacing
    pos = [t, 3 * t, 1023 * t, 2.0 ** -15, 2.0 ** -14,      # fp16 subnormals, the smallest normal
           0.5 * t, _above(0.5 * t), _below(0.5 * t),       # halfway between 0 and the smallest subnormal: to even (0); just off it
           1.5 * t, 2.5 * t, _above(2.5 * t), _below(1.5 * t), 1022.5 * t, 1023.5 * t,      # subnormal ties; 1023.5 t -> 2^-14
           1e-8, 6.0e-5, 6.1e-5,
           1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, _above(1.0 + 2.0 ** -11), _below(1.0 + 3 * 2.0 ** -11),   # ties at 1: down / up to even
           2049.0, 2051.0, _above(2049.0), _below(2051.0), 0.1 + 0.0, 1.0 / 3.0,
           65504.0, 65505.0, 65519.0, _below(65520.0),      # the largest fp16; just below the overflow threshold 65520
           _above(65504.0), 65488.0 + 8.0, 32767.99]
    return pos + [-v for v in pos] + [0.0]


@pytest.mark.parametrize('n', EW_SIZES)
def test_f32_to_f16(lib, n):
    """bit-equal to x.half() (round to nearest even): fp16 subnormals, ties, +-65504 and values just below the overflow threshold"""
    x = with_specials(rnd((n,), 101, 3.0), convert_specials())
    want = x.half()
    assert bool(torch.isfinite(want).all())
    xd = din(x)
    out = guarded_out((n,), torch.half)
    assert lib.fgdm_op_f32_to_f16(_p(xd), _p(out.t), n, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.numel() == 0, (n, int(bad[0]), float(x[int(bad[0])]), float(got[int(bad[0])]), float(want[int(bad[0])]))


@pytest.mark.parametrize('n', EW_SIZES)
def test_add_f16_to_f32(lib, n):
    """one fp32 add per element: bit-equal to a + b.float().  The stream carries per-element offsets of up to +-100, as the
    residual stream of a real CLIP checkpoint does."""
    a = rnd((n,), 102, 3.0) + 100.0 * (rnd((n,), 103) > 2.0) - 100.0 * (rnd((n,), 104) > 2.0)
    b = rnd((n,), 105, 3.0).half()
    want = a + b.float()
    ad, bd = din(a), din(b)
    out = guarded_out((n,), torch.float32)
    assert lib.fgdm_op_add_f16_to_f32(_p(ad), _p(bd), _p(out.t), n, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), n


# ================================================================================================== elementwise, bounded
@pytest.mark.parametrize('n', EW_SIZES)
def test_silu_f32_to_f16(lib, n):
    """silu_f (common.h) is one exp2, one add, one hardware reciprocal (1 ulp) and two multiplies in fp32: a few u of relative
    error, far below half an fp16 ulp (2^-11 relative).  So the stored value is the correctly rounded fp16 of the float64 result or
    its neighbour: |got - ref| <= ulp16(ref), ulp16 floored at the subnormal spacing 2^-24."""
    x = with_specials(uniform((n,), 106, -30.0, 30.0), [0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0])
    x64 = x.double()
    ref = x64 / (1.0 + torch.exp(-x64))
    xd = din(x)
    out = guarded_out((n,), torch.half)
    assert lib.fgdm_op_silu_f32_to_f16(_p(xd), _p(out.t), n, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().double().cpu()
    worst(f'silu_f32_to_f16 n {n}', (got - ref).abs(), ulp16(ref))


# ================================================================================================== embedding
VOCAB = 1000
EMBED_CASES = ((2 * 77, 77, 768), (3 * 5, 5, 1024), (71 * 77, 77, 768))


@pytest.mark.parametrize('rows,T,W', EMBED_CASES)
def test_embed_tokens(lib, rows, T, W):
    """one fp32 add per element: bit-equal to tok[clamp(ids)] + pos[t] in torch fp32.  Ids 0, vocab - 1, negative, >= vocab and
    beyond 32 bits, in the first and in the last rows; the position table has exactly T rows in front of its NaN guard.
    rows W / 4 = 1 049 664 > 4096 x 256 for (5467, 768): the grid-stride loop wraps."""
    tok, pos = rnd((VOCAB, W), 111), rnd((T, W), 112)
    g = torch.Generator().manual_seed(113)
    ids = torch.randint(0, VOCAB, (rows,), generator=g, dtype=torch.int64)
    edge = torch.tensor([0, VOCAB - 1, -3, VOCAB + 5, VOCAB, -1, 2 ** 32 + 7, -(2 ** 32) + 7], dtype=torch.int64)
    ids[:edge.numel()] = edge
    ids[-edge.numel():] = edge.flip(0)
    want = tok[ids.clamp(0, VOCAB - 1)] + pos[torch.arange(rows) % T]
    idd, tokd, posd = ids.cuda(), din(tok), din(pos)
    out = guarded_out((rows, W), torch.float32)
    assert lib.fgdm_op_embed_tokens(_p(idd), _p(tokd), _p(posd), _p(out.t), rows, T, W, VOCAB, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (rows, T, W)


# ================================================================================================== LayerNorm on fp32 rows
LN_ROWS = (1, 5, 154)
LN_WIDTHS = (4, 64, 252, 768, 1024, 1284)
LN_REGIMES = ('plain', 'large_mean', 'massive_channels')
LN_EPS = 1e-5


def ln_input(rows, C, regime):
    x = rnd((rows, C), 121, 1.5)
    if regime == 'plain':
        x = x + 0.3
    elif regime == 'large_mean':                # every row sits +-8 or +-32 standard deviations from zero
        shift = torch.tensor([8.0, -8.0, 32.0, -32.0])[torch.arange(rows) % 4]
        x = x + 1.5 * shift[:, None]
    else:                                       # two fixed channels carry 50 x the spread of the rest
        assert regime == 'massive_channels'
        x = x + 0.3
        x[:, C // 3] = rnd((rows,), 122, 75.0)
        x[:, C - 1] = rnd((rows,), 123, 75.0)
    return x.contiguous()


@functools.lru_cache(maxsize=None)
def ln_problem(rows, C, regime):
    """(x, gamma, beta, ref float64, bound float64 for the fp32 output): built once, shared by both output types"""
    x, gamma, beta = ln_input(rows, C, regime), 1.0 + rnd((C,), 124, 0.2), rnd((C,), 125, 0.1)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    mean = x64.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x64 - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xhat = (x64 - mean) * rstd
    ref = xhat * g64 + b64
    trips = -(-C // 256)
    assert trips <= 7           # see test_layernorm32: where the (d + 8) term covers the 4-per-trip chain of the variance
    d = trips + 10
    bound = 2 * U * (d * g64.abs() * rstd * x64.abs().mean(-1, keepdim=True) + (d + 8) * (g64 * xhat).abs() + ref.abs())
    return x, gamma, beta, ref, bound


@pytest.mark.parametrize('kind', ('f16', 'f32'))
@pytest.mark.parametrize('C', LN_WIDTHS)
def test_layernorm32(lib, C, kind):
    """ln32_kernel against float64 LayerNorm of the same fp32 rows, per element

        |got - ref| <= 2u [ d |gamma_c| rstd mean|x| + (d + 8) |gamma_c xhat_c| + |ref| ]  (+ ulp16(ref) / 2 for the fp16 output)

    with d = ceil(C / 256) + 10, read off norm.hip.  The kernel is two-pass, one wave per row, lane l walking c = 4 l + 256 k:
      mean   a value passes 3 adds inside its float4, ceil(C / 256) adds of the lane's running sum at most, 6 shuffle levels and
             the division by C: d roundings, so |mean^ - mean| <= d u mean|x|, which shifts the result by that times rstd |gamma_c|
             -- the first term; it is what grows with a row's offset (large-mean rows, massive channels).
      rstd   sum of (x - mean^)^2: the difference and the square (3 u), a chain of 4 ceil(C / 256) accumulations per lane (the
             four squares of a float4 are added one after the other, not as a float4 sum: deeper than the mean's chain), 6
             shuffle levels, the division, + eps: all terms positive, so (4 ceil(C / 256) + 11) u relative; half of it after the
             square root, plus the 1-ulp rsqrtf.  The error of mean^ enters the sum only in second order.
      value  (x - mean^) rstd gamma: three more roundings relative to |gamma_c xhat_c|; together with rstd
             (2 ceil(C / 256) + 10.5) u <= (d + 8) u for C <= 1792, every width here -- the second term.
      + beta one rounding of the result -- the third term.
    The factor 2 covers the second-order terms.  The same assertion serves all three input regimes, rows = 1, 5 (idle waves) and
    154, and both output types."""
    out_dtype = torch.half if kind == 'f16' else torch.float32
    for rows in LN_ROWS:
        for regime in LN_REGIMES:
            x, gamma, beta, ref, bound = ln_problem(rows, C, regime)
            xd, gd, bd = din(x), din(gamma), din(beta)
            out = guarded_out((rows, C), out_dtype)
            o16, o32 = (_p(out.t), None) if kind == 'f16' else (None, _p(out.t))
            assert lib.fgdm_op_layernorm32(_p(xd), rows, C, _p(gd), _p(bd), LN_EPS, o16, o32, _st()) == 0
            torch.cuda.synchronize()
            got = out.check().double().cpu()
            b = bound + 0.5 * ulp16(ref) if kind == 'f16' else bound
            worst(f'layernorm32 {kind} rows {rows} C {C} {regime}', (got - ref).abs(), b)


# ================================================================================================== first-stage 1x1 convolutions
VAE_SHAPES = ((1, 1), (3, 1000), (2, 4096), (3, 349613))          # 3 x 349 613 = 1 048 839 > 4096 x 256
VAE_SCALES = (1.0, 1.0 / 0.18215)
PERM4 = (2, 0, 3, 1)                    # no involutions: a transposed weight (co / ci swapped) is the inverse permutation
PERM8 = (3, 0, 6, 1, 7, 2, 4, 5)


def grid_values(shape, seed):
    """multiples of 2^-6 in [-8, 8]: fp16-representable, and exact in every sum with a bias that is a multiple of 1/4 below 4"""
    return (rnd(shape, seed, 2.0) * 64.0).round().clamp(-512, 512) / 64.0


def perm_wb(perm, bias):
    n = len(perm)
    w = torch.zeros(n, n)
    w[torch.arange(n), torch.tensor(perm)] = 1.0
    return torch.cat([w.reshape(-1), torch.tensor(bias)])


@pytest.mark.parametrize('scale', VAE_SCALES, ids=('scale 1', 'scale 1/0.18215'))
@pytest.mark.parametrize('B,HW', VAE_SHAPES)
def test_vae_prequant(lib, B, HW, scale):
    """z fp32 [B, 4, HW] -> fp16 [B, HW, 4].  The kernel rounds v = scale z, starts from the bias and adds the four products one
    after the other: at most 6 roundings on any term (v, the product, four sums; fewer where a product is fused), then the fp16
    store: |got - ref| <= 6u (|b| + sum |w| |scale z|) + ulp16(ref) / 2."""
    z, w, bias = rnd((B, 4, HW), 131, 1.2), rnd((4, 4), 132, 0.5), rnd((4,), 133, 0.3)
    s32 = float(torch.tensor(scale, dtype=torch.float32))           # the value the C ABI receives
    v = s32 * z.double()
    ref = torch.einsum('oi,bip->bpo', w.double(), v) + bias.double()
    mag = torch.einsum('oi,bip->bpo', w.double().abs(), v.abs()) + bias.double().abs()
    zd, wbd = din(z), din(torch.cat([w.reshape(-1), bias]))
    out = guarded_out((B, HW, 4), torch.half)
    assert lib.fgdm_op_vae_prequant(_p(zd), _p(wbd), scale, _p(out.t), B, HW, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().double().cpu()
    worst(f'vae_prequant B {B} HW {HW} scale {s32:.4f}', (got - ref).abs(), 6 * U * mag + 0.5 * ulp16(ref))


def test_vae_prequant_permutation_is_exact(lib):
    """a permutation weight, distinct biases, scale 1 and fp16-representable z: every product and sum is exact, so the output is,
    bit for bit, the permuted input plus the bias in NHWC order"""
    B, HW = 3, 1000
    bias = [0.5, -1.25, 2.0, -3.0]
    z = grid_values((B, 4, HW), 134)
    want = (z[:, list(PERM4), :] + torch.tensor(bias)[None, :, None]).permute(0, 2, 1).contiguous().half()
    zd, wbd = din(z), din(perm_wb(PERM4, bias))
    out = guarded_out((B, HW, 4), torch.half)
    assert lib.fgdm_op_vae_prequant(_p(zd), _p(wbd), 1.0, _p(out.t), B, HW, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize('B,HW', VAE_SHAPES)
def test_vae_moments(lib, B, HW):
    """h fp32 [B, HW, 8] -> fp32 [B, 8, HW].  The bias, then eight products added one after the other: at most 9 roundings on any
    term: |got - ref| <= 10u (|b| + sum |w| |h|)."""
    h, w, bias = rnd((B, HW, 8), 141, 1.5), rnd((8, 8), 142, 0.35), rnd((8,), 143, 0.3)
    ref = torch.einsum('oi,bpi->bop', w.double(), h.double()) + bias.double()[None, :, None]
    mag = torch.einsum('oi,bpi->bop', w.double().abs(), h.double().abs()) + bias.double().abs()[None, :, None]
    hd, wbd = din(h), din(torch.cat([w.reshape(-1), bias]))
    out = guarded_out((B, 8, HW), torch.float32)
    assert lib.fgdm_op_vae_moments(_p(hd), _p(wbd), _p(out.t), B, HW, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().double().cpu()
    worst(f'vae_moments B {B} HW {HW}', (got - ref).abs(), 10 * U * mag)


def test_vae_moments_permutation_is_exact(lib):
    """a permutation weight, distinct biases and inputs on a 2^-6 grid: every product and sum is exact, so the output is, bit for
    bit, the permuted input plus the bias in NCHW order"""
    B, HW = 3, 1000
    bias = [0.5, -1.25, 2.0, -3.0, 0.25, 1.75, -0.75, 3.5]
    h = grid_values((B, HW, 8), 144)
    want = (h[:, :, list(PERM8)] + torch.tensor(bias)).permute(0, 2, 1).contiguous()
    hd, wbd = din(h), din(perm_wb(PERM8, bias))
    out = guarded_out((B, 8, HW), torch.float32)
    assert lib.fgdm_op_vae_moments(_p(hd), _p(wbd), _p(out.t), B, HW, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
