"""Crop geometry and blending weights of the reference's patch-wise routes (`split_input_params`).

  plan     <-  LatentDiffusion.get_fold_unfold's crop count (ldm/models/diffusion/ddpm.py:718-722) and the kernel / stride
               clamping of decode_first_stage (ddpm.py:847-853)
  weights  <-  delta_border / get_weighting (ddpm.py:683-711)

Host code only (torch CPU ops, fp32): the tables are a few KiB, computed once per geometry and handed to the fold kernels
(csrc/patches.hip).  Crop l = ly * Lx + lx has its top-left corner at (ly * stride[0], lx * stride[1]): the column order of
torch.nn.Unfold."""
import torch

SPATIAL_COND_KEYS = ('image', 'LR_image', 'segmentation', 'bbox_img', 'coordinates_bbox')


def _pair(v, what):
    v = tuple(int(a) for a in v)
    if len(v) != 2:
        raise ValueError(f'split_input_params: {what} must have two entries, got {v}')
    return v


def plan(h, w, ks, stride, clamp=True):
    """((kh, kw), (sh, sw), Ly, Lx) of an h x w grid cut into ks crops every `stride` cells.

    clamp: kernel and stride are first reduced to the grid, per axis, as decode_first_stage does (ddpm.py:847-853).
    apply_model (ddpm.py:1049-1054) does not clamp: there a crop larger than the grid is an error.

    ValueError when the crops do not cover the grid: (h - kh) % sh != 0, (w - kw) % sw != 0, or a stride larger than the
    crop.  The reference folds such a grid without complaint, divides 0 by 0 in the cells no crop reaches and returns NaN
    pixels; this mirror refuses instead.  A crop of fewer than 2 cells along an axis is refused too: the border distance
    divides by (size - 1)."""
    kh, kw = _pair(ks, 'ks')
    sh, sw = _pair(stride, 'stride')
    h, w = int(h), int(w)
    if clamp:
        kh, kw = min(kh, h), min(kw, w)
        sh, sw = min(sh, h), min(sw, w)
    if kh < 2 or kw < 2:
        raise ValueError(f'split_input_params: crop {kh} x {kw} needs at least 2 cells per axis')
    if sh < 1 or sw < 1:
        raise ValueError(f'split_input_params: stride {(sh, sw)} must be positive')
    if kh > h or kw > w:
        raise ValueError(f'split_input_params: crop {kh} x {kw} is larger than the {h} x {w} grid')
    if sh > kh or sw > kw:
        raise ValueError(f'split_input_params: stride {(sh, sw)} larger than the crop {(kh, kw)} leaves cells uncovered')
    if (h - kh) % sh or (w - kw) % sw:
        raise ValueError(f'split_input_params: crops of {kh} x {kw} every {(sh, sw)} do not cover the {h} x {w} grid '
                         f'((size - ks) must be a multiple of the stride)')
    return (kh, kw), (sh, sw), (h - kh) // sh + 1, (w - kw) // sw + 1


def delta_border(h, w):
    """fp32 [h, w]: distance to the nearest border in units of the axis length, 0 on the border, 0.5 in the centre
    (ddpm.py:683-695: integer coordinates divided by (size - 1), then the minimum over y, x, 1 - y, 1 - x)."""
    y = (torch.arange(0, h).view(h, 1) / torch.tensor(h - 1)).expand(h, w)
    x = (torch.arange(0, w).view(1, w) / torch.tensor(w - 1)).expand(h, w)
    near = torch.minimum(y, x)
    far = torch.minimum(1 - y, 1 - x)
    return torch.minimum(near, far).to(torch.float32).contiguous()


def weights(kh, kw, Ly, Lx, params):
    """(w_pix fp32 [kh, kw], w_tie fp32 [Ly * Lx]) of get_weighting (ddpm.py:697-711): every cell of a crop weighs its clipped
    border distance; with `tie_braker` crop l additionally weighs the clipped border distance of its place in the Ly x Lx crop
    grid (else 1).  The reference's weighting[..., l] is w_pix * w_tie[l], rounded to fp32 once."""
    w_pix = torch.clip(delta_border(kh, kw), params['clip_min_weight'], params['clip_max_weight'])
    if params.get('tie_braker', False):
        w_tie = torch.clip(delta_border(Ly, Lx), params['clip_min_tie_weight'], params['clip_max_tie_weight']).reshape(Ly * Lx)
    else:
        w_tie = torch.ones(Ly * Lx, dtype=torch.float32)
    return w_pix.contiguous(), w_tie.contiguous()


def normalization(Ho, Wo, w_pix, w_tie, stride, Lx):
    """fp32 [Ho, Wo]: the folded weighting, summed over the covering crops in ascending l as the fold kernels do (the
    reference's torch.nn.Fold adds the same terms in another order: equal up to the rounding of at most a few additions)."""
    kh, kw = w_pix.shape
    sh, sw = stride
    out = torch.zeros(Ho, Wo, dtype=torch.float32)
    for l in range(w_tie.numel()):
        y0, x0 = (l // Lx) * sh, (l % Lx) * sw
        out[y0:y0 + kh, x0:x0 + kw] += w_pix * w_tie[l]
    return out


def decode_geometry(h, w, params):
    """Geometry of the patch-wise decode_first_stage (ddpm.py:841-855): ((kh, kw), (sh, sw), Ly, Lx, f) on the LATENT grid,
    f = vqf.  The reference sizes the upscaled fold with ks[0] on both axes (ddpm.py:738), so a non-square crop fails there
    with a shape error: ValueError here."""
    (kh, kw), st, Ly, Lx = plan(h, w, params['ks'], params['stride'])
    if kh != kw:
        raise ValueError(f'split_input_params: patch-wise decoding needs a square crop, got {kh} x {kw} '
                         '(the reference builds its upscaled fold with ks[0] on both axes)')
    return (kh, kw), st, Ly, Lx, int(params['vqf'])
