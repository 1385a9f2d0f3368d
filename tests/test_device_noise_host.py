"""Host side of the device noise (fgdm_loop_noise_set / fgdm_randn, include/fgdm.h), no GPU: the numpy restatement of the generator
(tests/device_noise_ref.py) against the Random123 known-answer vectors, the binding against the header, and the routing of
LatentDiffusion / DDIMSampler / PLMSSampler(device_noise=seed) with stand-in engines that record their calls -- one engine call
whatever the walk's length, no noise tensors, no host draws, the same (stream, walk position, sample) on both routes -- and
device_noise=None as before."""
import contextlib
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import device_noise_ref as ref
import kernel_stubs
from fgdm_amd import _lib, dist, models, samplers
from test_ancestral_loop_host import RecEngine, _header_struct, _lib_or_build
from test_ddim_loop_host import StubEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, TOK = 2, 8, 8, 77
SEED = 0x1234_5678_9ABC_DEF1


# ------------------------------------------------------------------------------------------------------------ the generator
KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('counter,key,want', KAT)
def test_restatement_reproduces_the_known_answer_vectors(counter, key, want):
    assert tuple(int(v) for v in ref.philox4x32_10(counter, key)) == want


def test_restatement_is_elementwise_and_counts_across_word_boundaries():
    c = ref.counter_blocks((0xFFFFFFFE, 0xFFFFFFFF, 0, 7), 4)
    assert [int(v) for v in c[0]] == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1] and [int(v) for v in c[1]] == [0xFFFFFFFF, 0xFFFFFFFF, 0, 0]
    assert [int(v) for v in c[2]] == [0, 0, 1, 1] and [int(v) for v in c[3]] == [7] * 4
    many = ref.philox4x32_10(c, (5, 9))
    for k in range(4):
        one = ref.philox4x32_10([int(w[k]) for w in c], (5, 9))
        assert [int(w[k]) for w in many] == [int(v) for v in one]


def test_normals_are_bounded_by_construction_and_use_the_documented_coordinates():
    z = ref.randn64(SEED, ref.STREAM_STEP, 3, 3, 4 * 8 * 8, first_sample=5)
    assert z.shape == (3, 256) and np.abs(z).max() <= 5.77
    worst = ref.box_muller64(np.array([[0, 0, 0, 0xFFFFFFFF]], dtype=np.uint32))       # u1 = 2^-24: the longest radius
    assert abs(worst[0, 0] - np.sqrt(48 * np.log(2))) < 1e-12 and np.abs(worst).max() <= 5.77
    # rows are global samples, a repeat row is sample 0, and step / stream are counter words of their own
    assert np.array_equal(z[1], ref.randn64(SEED, ref.STREAM_STEP, 3, 1, 256, first_sample=6)[0])
    rep = ref.randn64(SEED, ref.STREAM_STEP, 3, 3, 256, first_sample=5, repeat=True)
    assert np.array_equal(rep[0], rep[2]) and np.array_equal(rep[0], ref.randn64(SEED, ref.STREAM_STEP, 3, 1, 256)[0])
    assert not np.array_equal(z, ref.randn64(SEED, ref.STREAM_Q, 3, 3, 256, first_sample=5))
    assert not np.array_equal(z, ref.randn64(SEED, ref.STREAM_STEP, 4, 3, 256, first_sample=5))
    assert not np.array_equal(z, ref.randn64(SEED + (1 << 32), ref.STREAM_STEP, 3, 3, 256, first_sample=5))


# ------------------------------------------------------------------------------------------------------------ binding and header
def test_binding_header_and_library_declare_the_plan_and_the_entries():
    lib = _lib_or_build()
    for entry in ('fgdm_loop_noise_set', 'fgdm_randn', 'fgdm_op_rand_bits'):
        assert getattr(lib, entry) is not None and entry in _lib.SIGNATURES
    cls = _lib.FgdmNoisePlan
    assert _lib.SIGNATURES['fgdm_loop_noise_set'][1][1]._type_ is cls
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    assert re.search(r'\bint\s+fgdm_loop_noise_set\s*\(\s*fgdm_engine\*\s*e,\s*const fgdm_noise_plan\*\s*plan\)\s*;', hdr)
    fields = _header_struct(hdr, 'fgdm_noise_plan')
    want = {'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'int32_t': C.c_int32, 'float': C.c_float}
    assert [f.rsplit(' ', 1)[1] for f in fields] == [n for n, _ in cls._fields_]
    assert [want[f.rsplit(' ', 1)[0]] for f in fields] == [t for _, t in cls._fields_]
    assert C.sizeof(cls) == 40 == int(re.search(r'#define FGDM_NOISE_PLAN_SIZE_V1 (\d+)', hdr).group(1))
    off = 0
    for fname, ftype in cls._fields_:           # natural alignment, no hole and no tail padding
        assert getattr(cls, fname).offset == off and off % C.sizeof(ftype) == 0, fname
        off += C.sizeof(ftype)
    assert off == 40 and cls.seed.offset == 8 and cls.first_sample.offset == 16 and cls.temperature.offset == 24
    assert (_lib.NOISE_STREAM_STEP, _lib.NOISE_STREAM_Q) == (ref.STREAM_STEP, ref.STREAM_Q) == (0, 1)
    doc = re.sub(r'(\s|\*)+', ' ', hdr)
    for word in ('ddim.py:265-268', 'ddpm.py:1295-1323', 'ddpm.py:342-345', 'noise_like', '0xD2511F53', '0xCD9E8D57', '0x9E3779B9',
                 '0xBB67AE85', '|z| <= 5.77'):
        assert word in doc, word
    # the existing loop structs have not grown
    assert C.sizeof(_lib.FgdmDdimParams) == 192 and C.sizeof(_lib.FgdmAncestralParams) == 176 and C.sizeof(_lib.FgdmPlmsParams) == 168


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib_or_build()
    p = _lib.FgdmNoisePlan()
    p.struct_size = C.sizeof(p)
    assert lib.fgdm_loop_noise_set(None, C.byref(p)) == -1 and lib.fgdm_loop_noise_set(None, None) == -1
    q = C.c_void_p(1 << 20)
    rn = lambda stream=0, step=0, first=0, out=q, b=2, per=256: lib.fgdm_randn(SEED, stream, step, first, 0, 1.0, out, b, per, None)
    assert rn(out=None) == -1 and rn(b=0) == -1 and rn(per=0) == -1 and rn(per=255) == -1 and rn(per=-4) == -1
    assert rn(stream=-1) == -1 and rn(step=-1) == -1 and rn(first=-1) == -1 and rn(first=2 ** 31 - 1) == -1
    assert lib.fgdm_op_rand_bits(SEED, 0, 0, 0, 0, None, 4, None) == -1 and lib.fgdm_op_rand_bits(SEED, 0, 0, 0, 0, q, 0, None) == -1


# ------------------------------------------------------------------------------------------------------------ routing
def gen_randn(seed, stream, step, shape, first_sample=0, repeat=False, temperature=1., device=None):
    """Engine.randn's stand-in: the restatement, rounded to fp32, times temperature in fp32"""
    z = torch.from_numpy(ref.randn64(seed, stream, step, shape[0], int(np.prod(shape[1:])), first_sample, repeat).astype(np.float32))
    return (z * torch.tensor(temperature, dtype=torch.float32)).view(*shape)


class Armable:
    """loop_noise of a stand-in engine: records every plan; `armed` is the open one"""
    armed = None

    @contextlib.contextmanager
    def loop_noise(self, seed, first_sample=0, first_step=0, temperature=1., repeat_noise=False):
        self.armed = dict(seed=seed, first_sample=first_sample, first_step=first_step, temperature=temperature, repeat_noise=repeat_noise)
        self.plans.append(self.armed)
        try:
            yield self
        finally:
            self.armed = None


class SeededEngine(Armable, RecEngine):
    """RecEngine whose sample_ancestral, while armed, makes the planes it is not handed -- as the armed library does in its kernel"""

    def __init__(self):
        super().__init__()
        self.plans, self.handed = [], []

    def sample_ancestral(self, x_T, cond, timesteps, tables, **kw):
        self.handed.append(dict(kw, armed=self.armed))
        a = self.armed
        if a is not None:
            S = len(timesteps)
            if kw.get('step_noise') is None:
                kw['step_noise'] = torch.stack([gen_randn(a['seed'], ref.STREAM_STEP, a['first_step'] + i, x_T.shape, a['first_sample'],
                                                          a['repeat_noise'], a['temperature']) for i in range(S)])
            if kw.get('mask') is not None and kw.get('q_noise') is None:
                kw['q_noise'] = torch.stack([gen_randn(a['seed'], ref.STREAM_Q, a['first_step'] + i, x_T.shape, a['first_sample'])
                                             for i in range(S)])
        return super().sample_ancestral(x_T, cond, timesteps, tables, **kw)


class SeededStub(Armable, StubEngine):
    def __init__(self, n_controlnets=0):
        super().__init__(n_controlnets)
        self.plans = []

    def sample_ddim_ex(self, *a, **kw):
        out = super().sample_ddim_ex(*a, **kw)
        self.loops[-1]['armed'] = self.armed
        return out

    def sample_plms(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, **kw):
        self.loops.append(dict(kw, armed=self.armed, entry='plms'))
        z = torch.zeros(len(kw.get('log_steps', ())), *x_T.shape)
        return x_T.clone(), z, z.clone()


@pytest.fixture()
def host(monkeypatch):
    """the kernels' torch stand-ins plus the generator's; every torch draw and every generator draw recorded in order"""
    seen = types.SimpleNamespace(torch=[], gen=[])
    k = types.SimpleNamespace(**{n: getattr(kernel_stubs, n) for n in dir(kernel_stubs) if not n.startswith('_')})

    def randn(seed, stream, step, shape, first_sample=0, repeat=False, temperature=1., device=None):
        seen.gen.append((seed, stream, step, tuple(shape), first_sample, bool(repeat), temperature))
        return gen_randn(seed, stream, step, shape, first_sample, repeat, temperature)

    def t_randn(shape, device):
        seen.torch.append(('randn', tuple(shape)))
        return torch.randn(shape)

    def t_randn_like(x, **kw):
        seen.torch.append(('randn_like', tuple(x.shape)))
        return torch.randn(x.shape)
    k.randn = randn
    monkeypatch.setattr(samplers, '_k', k)
    monkeypatch.setattr(models, '_k', k)
    monkeypatch.setattr(samplers, '_randn', t_randn)
    monkeypatch.setattr(models, '_randn', t_randn)
    monkeypatch.setattr(torch, 'randn_like', t_randn_like)
    return seen


def _inputs(seed=3, b=B):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(b, 4, H, W), r(b, TOK, 8), r(b, 4, H, W)


MASK = (torch.arange(H) % 2 == 0).float().view(1, 1, H, 1)


@pytest.mark.parametrize('masked,repeat,temperature', [(False, False, 1.0), (True, False, 1.0), (True, True, 0.7)])
def test_seeded_ancestral_is_one_call_without_tensors_or_host_draws_and_both_routes_agree(host, masked, repeat, temperature):
    x_T, c, x0 = _inputs()
    S = 6
    kw = dict(x_T=x_T, timesteps=S, return_intermediates=True, log_every_t=2, temperature=temperature)
    if masked:
        kw.update(mask=MASK, x0=x0)
    if repeat:
        kw.update(repeat_noise=True)
    m = models.LatentDiffusion(engine=SeededEngine(), use_adapter=False, device_loop=True, device_noise=SEED)
    m.max_loop_noise_bytes = B * 4 * H * W * 4                  # the pre-drawn route would cut this walk into S (or 2 S) calls
    out, inter = m.p_sample_loop(c, (B, 4, H, W), **kw)
    assert len(m.engine.ancestral) == len(m.engine.handed) == 1 and not m.engine.calls
    k = m.engine.handed[0]
    assert k.get('step_noise') is None and k.get('q_noise') is None and (k['mask'] is not None) == masked
    assert k['armed'] == dict(seed=SEED, first_sample=0, first_step=0, temperature=1., repeat_noise=repeat)      # std carries the temperature
    assert m.engine.armed is None and m.engine.ancestral[0]['timesteps'] == [5, 4, 3, 2, 1, 0]
    assert host.torch == [] and host.gen == []                  # nothing drawn on the host, by either generator
    # the per-step route with the same seed: the same numbers at the same (stream, walk position), so the same trajectory
    m2 = models.LatentDiffusion(engine=SeededEngine(), use_adapter=False, device_noise=SEED)
    ref_out, ref_inter = m2.p_sample_loop(c, (B, 4, H, W), **kw)
    assert not m2.engine.ancestral and len(m2.engine.calls) == S and host.torch == []
    per_step = [(SEED, ref.STREAM_STEP, i, (B, 4, H, W), 0, repeat, 1.) for i in range(S)]
    if masked:
        per_step = [d for i, s in enumerate(per_step) for d in (s, (SEED, ref.STREAM_Q, i, (B, 4, H, W), 0, False, 1.))]
    assert host.gen == per_step
    assert torch.equal(out, ref_out) and not torch.equal(out, x_T)
    assert len(inter) == len(ref_inter) and all(torch.equal(a, b) for a, b in zip(inter, ref_inter))


def test_a_shard_draws_the_rows_of_the_whole_batch(host):
    x_T, c, x0 = _inputs(b=4)
    kw = dict(timesteps=4, mask=MASK, x0=None)
    whole = models.LatentDiffusion(engine=SeededEngine(), use_adapter=False, device_loop=True, device_noise=SEED)
    full = whole.p_sample_loop(c, (4, 4, H, W), x_T=x_T, **dict(kw, x0=x0))
    for rank in range(2):
        for loop in (True, False):
            m = models.LatentDiffusion(engine=SeededEngine(), use_adapter=False, device_loop=loop, device_noise=SEED)
            lo = dist.shard_device_noise(m, 4, rank, 2)
            assert lo == 2 * rank == m.noise_first_sample
            part = m.p_sample_loop(dist.shard(c, rank, 2), (2, 4, H, W), x_T=dist.shard(x_T, rank, 2), **dict(kw, x0=dist.shard(x0, rank, 2)))
            assert torch.equal(part, full[lo:lo + 2])
            if loop:
                assert m.engine.handed[0]['armed']['first_sample'] == lo


def test_without_a_seed_the_calls_and_draws_are_those_of_before(host):
    x_T, c, x0 = _inputs()
    S = 5
    m = models.LatentDiffusion(engine=SeededEngine(), use_adapter=False, device_loop=True)
    assert m.device_noise is None and m.noise_first_sample == 0
    m.max_loop_noise_bytes = 2 * 2 * B * 4 * H * W * 4
    torch.manual_seed(11)
    m.p_sample_loop(c, (B, 4, H, W), x_T=x_T, timesteps=S, mask=MASK, x0=x0)
    assert host.torch == [('randn', (B, 4, H, W)), ('randn_like', (B, 4, H, W))] * S and host.gen == [] and m.engine.plans == []
    assert [k['timesteps'] for k in m.engine.ancestral] == [[4, 3], [2, 1], [0]]
    assert all(tuple(k['step_noise'].shape[1:]) == (B, 4, H, W) == tuple(k['q_noise'].shape[1:]) and k['armed'] is None for k in m.engine.handed)
    for cls in (samplers.DDIMSampler, samplers.PLMSSampler, samplers.ControlDDIMSampler):
        s = cls(models.LatentDiffusion(engine=SeededStub(), use_adapter=False), device_loop=True)
        assert s.device_noise is None and s.noise_first_sample == 0
    del host.torch[:]
    s = samplers.DDIMSampler(models.LatentDiffusion(engine=SeededStub(), use_adapter=False), device_loop=True)
    torch.manual_seed(11)
    s.sample(4, B, (4, H, W), c, verbose=False, eta=1.0, x_T=x_T, mask=MASK, x0=x0)
    k = s.model.engine.loops[0]
    assert host.torch == [('randn_like', (B, 4, H, W)), ('randn', (B, 4, H, W))] * 4 and host.gen == [] and s.model.engine.plans == []
    assert tuple(k['step_noise'].shape) == tuple(k['q_noise'].shape) == (4, B, 4, H, W) and k['armed'] is None


@pytest.mark.parametrize('cls', [samplers.DDIMSampler, samplers.ControlDDIMSampler])
@pytest.mark.parametrize('masked', [False, True])
def test_seeded_ddim_hands_over_no_noise_and_the_per_step_route_uses_the_walk_positions(host, cls, masked, temperature=0.8):
    x_T, c, x0 = _inputs()
    control = cls is samplers.ControlDDIMSampler
    make = lambda: (models.ControlLDM(engine=SeededStub(1), n_controlnets=1) if control else
                    models.LatentDiffusion(engine=SeededStub(), use_adapter=False))
    cond = {'c_crossattn': [c], 'c_concat': None} if control else c
    kw = dict(verbose=False, eta=1.0, x_T=x_T, temperature=temperature)
    if masked:
        kw.update(mask=MASK, x0=x0)
    s = cls(make(), device_loop=True, device_noise=SEED)
    s.noise_first_sample = 4
    s.sample(4, B, (4, H, W), cond, **kw)
    eng = s.model.engine
    assert len(eng.loops) == 1 and not eng.calls and host.torch == [] and host.gen == []
    k = eng.loops[0]
    assert k.get('step_noise') is None and k.get('q_noise') is None and np.asarray(k['sigmas']).all()
    assert k['armed'] == dict(seed=SEED, first_sample=4, first_step=0, temperature=temperature, repeat_noise=False)
    assert ('mask' in k) == masked and eng.armed is None
    # per-step: q_sample's noise of the blend in front of step i, then the step's, both at walk position i
    s2 = cls(make(), device_noise=SEED)
    s2.noise_first_sample = 4
    s2.sample(4, B, (4, H, W), cond, **kw)
    assert len(s2.model.engine.calls) == 4 and not s2.model.engine.loops and host.torch == []
    want = []
    for i in range(4):
        if masked:
            want.append((SEED, ref.STREAM_Q, i, (B, 4, H, W), 4, False, 1.))
        want.append((SEED, ref.STREAM_STEP, i, (B, 4, H, W), 4, False, temperature))
    assert host.gen == want


def test_seeded_plms_hands_over_no_q_noise(host):
    x_T, c, x0 = _inputs()
    s = samplers.PLMSSampler(models.LatentDiffusion(engine=SeededStub(), use_adapter=False), device_loop=True, device_noise=SEED)
    s.sample(4, B, (4, H, W), c, verbose=False, x_T=x_T, mask=MASK, x0=x0)
    k = s.model.engine.loops[0]
    assert k['entry'] == 'plms' and k['q_noise'] is None and k['mask'] is not None and host.torch == [] and host.gen == []
    assert k['armed'] == dict(seed=SEED, first_sample=0, first_step=0, temperature=1., repeat_noise=False)
    s2 = samplers.PLMSSampler(models.LatentDiffusion(engine=SeededStub(), use_adapter=False), device_noise=SEED)
    s2.sample(4, B, (4, H, W), c, verbose=False, x_T=x_T, mask=MASK, x0=x0)
    assert host.gen == [(SEED, ref.STREAM_Q, i, (B, 4, H, W), 0, False, 1.) for i in range(4)] and host.torch == []
