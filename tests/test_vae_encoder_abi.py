"""First-stage encoder, host side (no GPU): the parameter table of an engine built with `vae_encoder` is the reference's whole
AutoencoderKL.state_dict() in order (tests/golden/vae_encoder_keys.json), the switch is opt-in and appended to the config struct
without moving any earlier field, the two new entry points are exported, and DiagonalGaussianDistribution on CPU tensors
evaluates the closed forms of ldm/modules/distributions/distributions.py:24-63."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import golden_inputs as gi
from fgdm_amd import _lib, engine as eng, models

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FS = 'first_stage_model.'


def _first_stage(shapes):
    return {k: tuple(v) for k, v in shapes.items() if k.startswith(FS)}


def test_param_table_with_encoder_is_the_whole_autoencoder():
    ref = json.load(open(os.path.join(GOLD, 'vae_encoder_keys.json')))
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, vae=True, vae_encoder=True))
    fs = _first_stage(got)
    assert list(fs) == list(ref)
    assert all(tuple(ref[k]) == v for k, v in fs.items())
    assert list(got)[-len(fs):] == list(fs)          # the first stage still follows the UNet
    # registration order of autoencoder.py:298-303
    heads = [k[len(FS):].split('.')[0] for k in fs]
    assert [h for i, h in enumerate(heads) if i == 0 or heads[i - 1] != h] == ['encoder', 'decoder', 'quant_conv', 'post_quant_conv']
    # ... and without the encoder's own keys it is exactly the decoder-only table
    dec = json.load(open(os.path.join(GOLD, 'param_keys.json')))['vae_decoder']
    rest = {k: v for k, v in fs.items() if not k.startswith((FS + 'encoder.', FS + 'quant_conv.'))}
    assert list(rest) == list(dec)
    assert all(tuple(dec[k]) == v for k, v in rest.items())


def test_param_table_without_encoder_is_unchanged():
    dec = json.load(open(os.path.join(GOLD, 'param_keys.json')))['vae_decoder']
    for kw in (dict(vae=True), dict(vae=True, vae_encoder=False)):
        got = eng.param_shapes(eng.make_config(gi.SD_CFG, **kw))
        fs = _first_stage(got)
        assert list(fs) == list(dec)
        assert all(tuple(dec[k]) == v for k, v in fs.items())
    plain = eng.param_shapes(eng.make_config(gi.SD_CFG))
    assert not _first_stage(plain)
    assert eng.make_config(gi.SD_CFG, vae=True).vae_encoder == 0
    assert eng.make_config(gi.SD_CFG, vae=True, vae_encoder=True).vae_encoder == 1


def test_unsupported_encoder_configs_are_rejected():
    with pytest.raises(ValueError):
        eng.make_config(gi.SD_CFG, vae_encoder=True)                       # no first-stage config at all
    with pytest.raises(ValueError):
        eng.make_config(gi.SD_CFG, vae=dict(eng.SD_VAE, attn_resolutions=[32]), vae_encoder=True)
    with pytest.raises(ValueError):
        eng.param_shapes(eng.make_config(gi.SD_CFG, vae=dict(eng.SD_VAE, ch=96), vae_encoder=True))
    c = eng.make_config(gi.SD_CFG)          # the C side checks too: the flag without vae_ch, and values other than 0 / 1
    c.vae_encoder = 1
    with pytest.raises(ValueError):
        eng.param_shapes(c)
    c = eng.make_config(gi.SD_CFG, vae=True)
    c.vae_encoder = 2
    with pytest.raises(ValueError):
        eng.param_shapes(c)


def test_config_struct_grows_by_one_trailing_field():
    names = [f[0] for f in _lib.FgdmConfig._fields_]
    assert names[-1] == 'vae_encoder' and names[-2] == 'n_extra_adapters'
    assert _lib.FgdmConfig._fields_[-1][1] is C.c_int32

    class Parent(C.Structure):          # the struct before the encoder existed: every field but the last
        _fields_ = _lib.FgdmConfig._fields_[:-1]
    for name in names[:-1]:
        assert getattr(_lib.FgdmConfig, name).offset == getattr(Parent, name).offset, name
    assert _lib.FgdmConfig.workspace_bytes.offset == 112 and _lib.FgdmConfig.n_extra_adapters.offset == 196
    assert _lib.FgdmConfig.vae_encoder.offset == 200
    assert C.alignment(_lib.FgdmConfig) == 8
    assert C.sizeof(_lib.FgdmConfig) == C.sizeof(Parent) + 8 == 208


def test_new_symbols_exported():
    lib = _lib.load()
    for name in ('fgdm_vae_encode', 'fgdm_posterior_sample'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(GOLD), '..', 'include', 'fgdm.h')).read()
    assert 'int32_t vae_encoder;' in hdr and 'FGDM_STRIDE2_PAD_BR' in hdr
    assert _lib.STRIDE2_PAD_BR == -2


def test_engine_args_switch_is_opt_in():
    a = models.LatentDiffusion.engine_args(first_stage_config=True)
    assert 'vae_encoder' not in a and a['vae'] is True
    a = models.LatentDiffusion.engine_args(first_stage_config=True, first_stage_encoder=True)
    assert a['vae_encoder'] is True
    a = models.ControlLDM.engine_args(first_stage_config=True, first_stage_encoder=True)
    assert a['vae_encoder'] is True and a['n_controlnets'] == 1


def _moments(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 8, 5, 6, generator=g) * torch.tensor([1.0] * 4 + [1.5] * 4).view(1, 8, 1, 1)


def test_distribution_closed_forms_cpu():
    p = _moments()
    d = models.DiagonalGaussianDistribution(p)
    mean, logvar = p[:, :4], p[:, 4:]
    assert d.parameters is p and not d.deterministic
    assert torch.equal(d.mean, mean) and torch.equal(d.logvar, logvar)          # nothing near the clamp here
    assert torch.equal(d.std, torch.exp(0.5 * logvar)) and torch.equal(d.var, torch.exp(logvar))
    torch.manual_seed(11)
    got = d.sample()
    torch.manual_seed(11)
    noise = torch.randn(mean.shape)
    assert torch.equal(got, mean + torch.exp(0.5 * logvar) * noise)
    assert torch.equal(d.mode(), mean)
    kl = 0.5 * (mean ** 2 + logvar.exp() - 1.0 - logvar).sum(dim=(1, 2, 3))
    torch.testing.assert_close(d.kl(), kl, rtol=1e-6, atol=1e-6)
    q = models.DiagonalGaussianDistribution(_moments(4))
    kl2 = 0.5 * ((mean - q.mean) ** 2 / q.var + d.var / q.var - 1.0 - logvar + q.logvar).sum(dim=(1, 2, 3))
    torch.testing.assert_close(d.kl(q), kl2, rtol=1e-6, atol=1e-6)
    x = _moments(5)[:, :4]
    nll = 0.5 * (math.log(2.0 * math.pi) + logvar + (x - mean) ** 2 / logvar.exp()).sum(dim=(1, 2, 3))
    torch.testing.assert_close(d.nll(x), nll, rtol=1e-6, atol=1e-6)


def test_distribution_clamp_and_deterministic_cpu():
    p = _moments()
    p[:, 4] = -50.0
    p[:, 5] = 40.0
    d = models.DiagonalGaussianDistribution(p)
    assert float(d.logvar[:, 0].max()) == -30.0 and float(d.logvar[:, 1].min()) == 20.0
    assert torch.equal(d.std[:, 0], torch.full_like(d.std[:, 0], math.exp(-15.0)))
    assert torch.equal(d.std[:, 1], torch.full_like(d.std[:, 1], math.exp(10.0)))
    assert torch.equal(d.logvar[:, 2:], p[:, 6:])
    det = models.DiagonalGaussianDistribution(p, deterministic=True)
    assert not det.std.any() and not det.var.any()
    torch.manual_seed(1)
    assert torch.equal(det.sample(), det.mean)
    assert float(det.kl()) == 0.0 and float(det.nll(det.mean)) == 0.0


def test_get_first_stage_encoding_branches_cpu():
    """ddpm.py:648-661 on CPU tensors, without an engine (the method reads scale_factor only)."""
    m = models.LatentDiffusion.__new__(models.LatentDiffusion)
    m.scale_factor = 0.18215
    p = _moments()
    d = models.DiagonalGaussianDistribution(p)
    torch.manual_seed(5)
    z = m.get_first_stage_encoding(d)
    torch.manual_seed(5)
    assert torch.equal(z, 0.18215 * d.sample())
    t = p[:, :4]
    assert torch.equal(m.get_first_stage_encoding(t), 0.18215 * t)
    torch.manual_seed(6)
    zz = m.get_first_stage_encoding([d, d])
    torch.manual_seed(6)
    assert torch.equal(zz, 0.18215 * torch.cat([d.sample(), d.sample()], 1))
    with pytest.raises(NotImplementedError):
        m.get_first_stage_encoding(3.0)


def test_dropin_maps_the_distribution():
    from fgdm_amd import dropin
    for name in ('ldm.modules.distributions.distributions', 'controlnet.ldm.modules.distributions.distributions'):
        assert dropin._MAP[name]['DiagonalGaussianDistribution'] is models.DiagonalGaussianDistribution


def test_synth_image_properties():
    from fgdm_amd import synth
    x = synth.image(2, 64, seed=64)
    assert x.shape == (2, 3, 64, 64) and x.dtype.name == 'float32'
    assert x.min() >= -1.0 and x.max() <= 1.0
    assert (x[0] != x[1]).any()
    assert (x == synth.image(2, 64, seed=64)).all()
    cell = x[0, 0, :8, :8]          # one palette cell: flat colour + 0.1 sigma texture
    assert 0.02 < cell.std() < 0.2
