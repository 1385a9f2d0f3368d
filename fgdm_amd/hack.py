"""controlnet/cldm/hack.py for the MI355X engine: the reference's long-prompt route.

  hack_everything(clip_skip)  <-  hack.py:23-68: FrozenCLIPEmbedder.forward encodes every prompt as three 75-token chunks, each
                                  wrapped in BOS / EOS and padded to 77, and hands the network a [B, 231, 768] context;
                                  clip_skip > 1 takes final_layer_norm(hidden_states[-clip_skip]) instead of last_hidden_state.
  disable_verbosity()         <-  hack.py:11-14
  enable_sliced_attention()   <-  hack.py:17-20,72-111: slices CrossAttention over (batch, head) to bound the score tensor.

The chunk layout is host code (plain lists of token ids); the transformer runs in the engine as ONE [3B, 77] batch
(fgdm_clip_encode_skip) whose rows (b f) are already the b (f i) layout of the result.  Only the BPE vocabulary stays outside:
`model.raw_tokenizer`, a callable list[str] -> list[list[int]] WITHOUT special tokens, truncation or padding."""
import torch

CHUNK = 75              # raw tokens per chunk (hack.py:47-48)
CHUNKS = 3
MAX_LENGTH = 77         # BOS + 75 + EOS
BOS, EOS, PAD = 49406, 49407, 49407      # openai/clip-vit-large-patch14, used when the tokenizer does not say

_STATE = {'enabled': False, 'clip_skip': 0}


def disable_verbosity():
    try:
        from transformers import logging
        logging.set_verbosity_error()
    except ImportError:      # the engine itself does not need the package
        pass
    print('logging improved.')


def enable_sliced_attention():
    """Nothing to switch: the engine's attention kernels keep the scores of a query tile in registers and never
    materialise the [B * heads, T, Tk] tensor whose size the reference's sliced forward bounds."""
    print('Sliced attention is not needed: the engine never materialises attention scores (no-op).')


def state():
    """(enabled, clip_skip) that models created from now on start with."""
    return _STATE['enabled'], _STATE['clip_skip']


def hack_everything(clip_skip=0, model=None):
    """Switch get_learned_conditioning to the chunked encoding: of `model` if one is given, else of every model created
    afterwards (the reference patches the FrozenCLIPEmbedder class before create_model, hack.py:23-28)."""
    disable_verbosity()
    if model is not None:
        model.clip_hack, model.clip_skip = True, int(clip_skip)
    else:
        _STATE['enabled'], _STATE['clip_skip'] = True, int(clip_skip)
    print('Enabled clip hacks.')


def chunk_tokens(raw_tokens, bos=BOS, eos=EOS, pad=PAD):
    """One prompt's raw token list -> three lists of 77 ids (hack.py:47-60): split at 75 and 150, tokens past 225 dropped,
    each chunk BOS + tokens + EOS, padded to 77 with PAD or cut to 77."""
    raw = list(raw_tokens)
    out = []
    for f in range(CHUNKS):
        x = [bos] + raw[CHUNK * f: CHUNK * (f + 1)] + [eos]
        out.append(x[:MAX_LENGTH] if len(x) >= MAX_LENGTH else x + [pad] * (MAX_LENGTH - len(x)))
    return out


def chunk_ids(raw_tokens_list, bos=BOS, eos=EOS, pad=PAD):
    """list of raw token lists -> int64 [B, 3, 77]"""
    return torch.tensor([chunk_tokens(r, bos, eos, pad) for r in raw_tokens_list], dtype=torch.int64).reshape(-1, CHUNKS, MAX_LENGTH)


def encode(engine, raw_tokens_list, clip_skip=0, bos=BOS, eos=EOS, pad=PAD):
    """_hacked_clip_forward after tokenisation (hack.py:53-68): [B, 231, 768] on the engine's device."""
    ids = chunk_ids(raw_tokens_list, bos, eos, pad)
    B = ids.shape[0]
    y = engine.clip_encode(ids.reshape(B * CHUNKS, MAX_LENGTH), clip_skip=clip_skip)     # 'b f i -> (b f) i'
    return y.reshape(B, CHUNKS * MAX_LENGTH, y.shape[-1])                                  # '(b f) i c -> b (f i) c'
