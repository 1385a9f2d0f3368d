"""Long text contexts without a GPU: the CPU oracle at 154 and 231 tokens against goldens from the reference's own modules
(tests/golden/long_context.npz), the chunk layout of the long-prompt route against the id arrays the reference's
_hacked_clip_forward feeds its transformer (tests/golden/clip_hack_tokens.json), the drop-in names of controlnet/cldm/hack.py,
the new C-ABI entries, and the samplers' handling of a prompt / negative prompt pair of different token counts."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import golden_inputs as gi
import long_context_inputs as li
from common import GOLD, gold, params, relerr
from fgdm_amd import hack, models, samplers
from oracle import arch, nn as onn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5     # fp32 vs fp32, different op order only: the bar of tests/test_oracle_golden.py


def test_oracle_unet_at_154_and_231_tokens():
    g = gold('long_context')
    p = params(arch.unet_param_shapes(gi.SD_CFG, adapter=True), 'model.diffusion_model.')
    t = torch.from_numpy(g['t'])
    assert t.tolist() == li.T
    with torch.no_grad():
        for tok in li.TOKENS:
            x, ctx = li.x(8), li.ctx(tok)
            assert tuple(ctx.shape) == (2, tok, 768)
            e = onn.unet_forward(p, gi.SD_CFG, x, t, ctx, prefix='model.diffusion_model.')
            assert relerr(e, g[f'eps_orig_{tok}']) < TOL, tok
            e = onn.unet_forward(p, gi.SD_CFG, x, t, ctx, prefix='model.diffusion_model.', use_adapter=True)
            assert relerr(e, g[f'eps_fgdm_{tok}']) < TOL, tok


def test_oracle_control_ldm_at_231_tokens():
    g = gold('long_context')
    p = params(arch.unet_param_shapes(gi.SD_CFG, adapter=False), 'model.diffusion_model.')
    p.update(params(arch.controlnet_param_shapes(gi.SD_CFG), 'control_model.'))
    with torch.no_grad():
        e = onn.control_ldm_apply(p, gi.SD_CFG, li.x(16), torch.from_numpy(g['t']), li.ctx(231), [li.hint(128)])
    assert relerr(e, g['eps_ctrl_231']) < TOL


def test_several_crossattn_parts_are_one_context_for_the_oracle():
    """cat(c_crossattn, 1) of three 77-token parts is the 231-token context (ddpm.py:1835-1837)"""
    ctx = li.ctx(231)
    parts = [ctx[:, 77 * i: 77 * (i + 1)].contiguous() for i in range(3)]
    m = models.LatentDiffusion.__new__(models.LatentDiffusion)
    joined = m._context({'c_crossattn': parts})
    assert torch.equal(joined, ctx)
    assert m._context(parts) is joined                   # same part objects: the SAME joined tensor (the engine's cache key)
    assert m._context([ctx]) is ctx
    parts[1].mul_(1.0)                                   # in-place write: joined anew
    assert m._context(parts) is not joined


def _cases():
    return json.load(open(os.path.join(GOLD, 'clip_hack_tokens.json')))


def test_chunk_layout_matches_the_reference():
    g = _cases()
    assert [c['raw_length'] for c in g['cases']] == list(li.RAW_LENGTHS)
    for c in g['cases']:
        raw = li.raw_tokens(c['raw_length'])
        assert hack.chunk_tokens(raw, g['bos'], g['eos'], g['pad']) == c['ids'], c['raw_length']
    ids = hack.chunk_ids([li.raw_tokens(n) for n in li.RAW_LENGTHS])
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (len(li.RAW_LENGTHS), 3, 77)
    assert ids.tolist() == [c['ids'] for c in g['cases']]


class _RecordingEngine:
    """stands in for the HIP engine: records the ids it is asked to encode, returns the ids as 1-wide "embeddings" """
    has_clip = True
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def clip_encode(self, ids, clip_skip=0):
        ids = torch.as_tensor(ids)
        self.calls.append((tuple(ids.shape), clip_skip))
        return ids.float().unsqueeze(-1)


def test_hack_everything_switches_get_learned_conditioning():
    g = _cases()
    raws = {f'prompt {n}': li.raw_tokens(n) for n in li.RAW_LENGTHS}
    want = torch.tensor([c['ids'] for c in g['cases']]).reshape(len(raws), 231, 1).float()
    saved = dict(hack._STATE)
    try:
        eng = _RecordingEngine()
        before = models.LatentDiffusion(engine=eng, use_adapter=False)
        assert not before.clip_hack
        hack.hack_everything(clip_skip=2)
        after = models.LatentDiffusion(engine=eng, use_adapter=False)
        assert after.clip_hack and after.clip_skip == 2 and not before.clip_hack      # models created afterwards
        after.raw_tokenizer = lambda prompts: [raws[p] for p in prompts]
        z = after.get_learned_conditioning(list(raws))
        assert eng.calls == [((3 * len(raws), 77), 2)]                # ONE [3B, 77] batch, clip_skip handed on
        assert tuple(z.shape) == (len(raws), 231, 1) and torch.equal(z, want)       # 'b (f i) c'
        # ready-made chunk ids take the same route
        assert torch.equal(after.get_learned_conditioning(hack.chunk_ids(list(raws.values()))), want)
        # a model passed in is switched on its own
        hack._STATE.update(saved)
        other = models.LatentDiffusion(engine=eng, use_adapter=False)
        assert not other.clip_hack
        hack.hack_everything(clip_skip=0, model=other)
        assert other.clip_hack and other.clip_skip == 0 and hack.state() == (saved['enabled'], saved['clip_skip'])
    finally:
        hack._STATE.update(saved)


def test_raw_tokenizer_missing_files_message():
    m = models.LatentDiffusion(engine=_RecordingEngine(), use_adapter=False)
    m.clip_hack = True
    m.clip_version = os.path.join(ROOT, 'no-such-tokenizer-directory')
    with pytest.raises(RuntimeError, match='model.raw_tokenizer'):
        m.get_learned_conditioning(['a bedroom'])


def test_hack_names_resolve_through_dropin(capsys):
    import fgdm_amd.dropin as dropin
    dropin.install()
    from controlnet.cldm.hack import disable_verbosity, enable_sliced_attention, hack_everything
    import cldm.hack as bare
    assert hack_everything is hack.hack_everything and bare.hack_everything is hack.hack_everything
    assert disable_verbosity is hack.disable_verbosity and bare.enable_sliced_attention is hack.enable_sliced_attention
    enable_sliced_attention()
    assert 'no-op' in capsys.readouterr().out


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_new_abi_entries_declared_and_exported(lib):
    from fgdm_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    declared = set(re.findall(r'\b(fgdm_[a-z0-9_]+)\s*\(', hdr))
    for name in ('fgdm_set_context_tokens', 'fgdm_get_context_tokens', 'fgdm_clip_encode_skip'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # each cites the reference lines it serves
    assert 'ddpm.py:1835-1837' in hdr and 'cldm.py:836-849' in hdr and 'hack.py:40-45' in hdr
    # argument checks that need no engine (no GPU here: an engine cannot be created, tests/test_lib_abi.py); the refusal of
    # tokens < 1 on a live engine is asserted in tests/test_gpu_long_context.py
    assert lib.fgdm_set_context_tokens(None, 0) < 0 and lib.fgdm_set_context_tokens(None, 231) < 0
    assert lib.fgdm_get_context_tokens(None) < 0
    assert lib.fgdm_clip_encode_skip(None, None, 1, 77, 2, None, None) < 0


def test_batched_cond_is_none_for_unequal_token_counts():
    """A 231-token prompt against a 77-token negative prompt cannot share one batch: two calls per step, as
    ddim_hacked.py:190-191 always does; the root samplers fail as the reference's torch.cat([uc, c]) fails."""
    c, uc, uc231 = li.ctx(231), li.ctx(77), li.ctx(231) * 0.5
    hint = li.hint(64)
    smp = samplers.ControlDDIMSampler.__new__(samplers.ControlDDIMSampler)
    cond = {'c_concat': [hint], 'c_crossattn': [c]}
    assert smp._batched_cond({'c_concat': [hint], 'c_crossattn': [uc]}, cond) is None
    both = smp._batched_cond({'c_concat': [hint], 'c_crossattn': [uc231]}, cond)
    assert tuple(both['c_crossattn'][0].shape) == (4, 231, 768)
    for cls in (samplers.DDIMSampler, samplers.PLMSSampler):
        root = cls.__new__(cls)
        with pytest.raises(RuntimeError):
            root._batched_cond(uc, c)
        assert tuple(root._batched_cond(uc231, c).shape) == (4, 231, 768)
