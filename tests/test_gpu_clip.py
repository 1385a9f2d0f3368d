"""Text encoder parity through the C ABI (fgdm_clip_encode): HIP engine vs transformers.CLIPTextModel with the same
synthetic weights (tests/golden/clip.npz; clip_ac.npz = the same model under the reference's autocast policy) and vs the
CPU oracle.  Tolerance max(1e-3, 1.1 x floor), floor = |autocast golden - fp32 golden| (tests/common.py: check_net)."""
import pytest
import torch

import golden_inputs as gi
from common import CAP_EVAL, NET_K, check_net, check_net_vs_oracle, gold, net_tol, params, relerr, report
from fgdm_amd import synth

pytestmark = pytest.mark.gpu



@pytest.fixture(scope='module')
def engine():
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, clip=True)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    yield e
    e.close()


def test_clip_encode_vs_transformers_golden(engine):
    g, ga = gold('clip'), gold('clip_ac')
    z = engine.clip_encode(gi.clip_ids())
    assert tuple(z.shape) == (2, 77, 768)
    # the engine keeps CLIP's hidden states as an fp32 residual stream, exactly where the reference's autocast does (fp32
    # embeddings; fp16 branch outputs promote when added) -- round 1 stored them as fp16 and sat at 1.4 x the floor
    check_net('clip text encoder (transformers)', z.cpu(), g['z'], ga['z'])


def test_clip_encode_batch_and_short_sequences(engine):
    """Per-prompt results do not depend on the batch; a causal model's prefix does not depend on what follows."""
    from oracle import clip as oclip
    ids = gi.clip_ids(5, seed=9)
    z = engine.clip_encode(ids)
    for b in range(5):
        assert torch.equal(engine.clip_encode(ids[b:b + 1])[0], z[b]), b
    short = engine.clip_encode(ids[:, :32])
    assert relerr(short.cpu(), z[:, :32].cpu()) < 1e-6
    p = params(oclip.param_shapes())
    with torch.no_grad():
        want = oclip.text_encode(p, ids)
    tol = net_tol(relerr(gold('clip_ac')['z'].astype('float32'), gold('clip')['z']))
    assert report('clip text encoder B=5 vs oracle', relerr(z.cpu(), want), tol) < tol


def test_get_learned_conditioning_mirror(engine):
    from fgdm_amd.models import LatentDiffusion
    m = LatentDiffusion(engine=engine, use_adapter=False)
    ids = gi.clip_ids()
    m.tokenizer = lambda prompts: ids[:len(prompts)]          # stand-in for the BPE tokenizer (no vocabulary files offline)
    c = m.get_learned_conditioning(['a photo of a cat', 'a bedroom'])
    assert torch.equal(c, engine.clip_encode(ids))
    assert torch.equal(m.get_learned_conditioning(ids), c)


MASSIVE_CHANNELS = (133, 587)
MASSIVE_OFFSET_STDS = 100


def test_clip_encode_with_massive_channels():
    """The residual stream of a real CLIP checkpoint carries a few channels with a large constant offset through every layer; the
    synthetic weights give O(1) hidden states only.  Here token_embedding.weight and position_embedding.weight get a constant
    added in two fixed channels (+off in channel 133, -off in channel 587, in both tables: the hidden state starts at +-2 off
    there, against a spread of 0.05 elsewhere), and the engine is judged like every network: against oracle.clip.text_encode on
    the same parameters, within net_tol(floor) of its fp32 mode, the floor measured on these inputs and capped at CAP_EVAL.
    off = 100 standard deviations of token_embedding.weight (0.03609: off = 3.609), the largest of 10, 30 and 100 for which the
    oracle's own floor stays below CAP_EVAL / NET_K = 3.67e-3: the floors are 7.44e-4, 7.21e-4 and 7.10e-4 (no offset: 8.98e-4)."""
    from fgdm_amd.engine import Engine
    from oracle import clip as oclip
    e = Engine(gi.SMALL_CFG, clip=True)
    try:
        p = params(oclip.param_shapes())
        tok, pos = (oclip.PREFIX + f'embeddings.{n}_embedding.weight' for n in ('token', 'position'))
        off = MASSIVE_OFFSET_STDS * float(p[tok].std())
        for k in (tok, pos):
            p[k] = p[k].clone()
            p[k][:, MASSIVE_CHANNELS[0]] += off
            p[k][:, MASSIVE_CHANNELS[1]] -= off
        for k, shape in e.param_shapes().items():
            e.load_tensor(k, p[k] if k in p else synth.make_tensor(k, shape))
        e.finalize()
        ids = gi.clip_ids()
        z = e.clip_encode(ids).cpu()
    finally:
        e.close()
    assert tuple(z.shape) == (2, 77, 768)
    _, floor = check_net_vs_oracle(f'clip text encoder, massive channels (offset {off:.3f})', z, lambda: oclip.text_encode(p, ids))
    assert floor < CAP_EVAL / NET_K, floor
