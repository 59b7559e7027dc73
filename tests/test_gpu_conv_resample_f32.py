"""GPU: the fp32 DownSample / UpSample convs (idf_conv_resample_f32), forward and data gradient, through ops.conv_raw /
ops.conv_dgrad_raw against float64 F.conv2d (stride 2, pad 1) / F.conv2d over the nearest x2 up-sampled input and their
autograd data gradients, at the project's fp32 bound.  Cases are (B, K, H, W, N) with H x W the low-resolution map (UP2
input, S2 output), K the channels the kernel sums over and N its output rows: the conv's (Cin, Cout) for the forward ops
and its (Cout, Cin) for the data gradients, so that the ragged row tiles and the chunk counts of a case reach all four."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL = 2e-5      # tests/test_gpu_kernels.py TOL[torch.float32]

CASES = [
    (2, 32, 4, 4, 64),          # smallest map, one chunk pair
    (3, 32, 5, 6, 32),          # odd height, W not a multiple of 4, odd batch
    (2, 64, 8, 16, 20), (2, 64, 16, 8, 72),     # H != W both ways, a ragged cout tile, a full tile plus a ragged one
    (2, 96, 8, 8, 64),          # 6 chunks: both slab buffers many times; the 16-pixel group wraps rows
    (2, 32, 10, 16, 32),        # the last row tile of an image masks rows
    (2, 64, 32, 32, 128),       # widest map, two cout tiles
    (32, 128, 8, 8, 128),       # a step shape: sub-pixel classes one per workgroup at a chip-filling batch
    (16, 64, 32, 32, 64),       # sub-pixel classes two per workgroup; 32-pixel tiles in the UP2 data gradient
    (32, 64, 32, 32, 64),       # a step shape: all four classes in one workgroup; 64-pixel tiles in the UP2 data gradient
]
OPS = ['s2_fwd', 's2_dgrad', 'up2_fwd', 'up2_dgrad']
# the S2 forward alone: odd Hs and Ws (9 x 11 -> 5 x 6), the right / bottom taps fall outside
# measured out of the predicate (profiles/f32_resample.txt): S2 forward launches that fill the chip, and the UP2 data
# gradient of the 8 x 8 map at the training batch -- the parent's route keeps them
GATED = [('s2_fwd', (16, 64, 32, 32, 64)), ('s2_fwd', (32, 64, 32, 32, 64)), ('up2_dgrad', (32, 128, 8, 8, 128))]
PARAMS = [(op, c) for op in OPS for c in CASES if (op, c) not in GATED] + [('s2_fwd_odd', (2, 32, 5, 6, 32))]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=2)
def _reference(op, case):
    """(conv input, weight, bias, residual shaped as the op's output, gradient fed to a dgrad op, float64 result)."""
    B, Cin, H, W, Cout = case if not op.endswith('dgrad') else (case[0], case[4], case[2], case[3], case[1])
    up = op.startswith('up2')
    Hs, Ws = (H, W) if up else ((2 * H - 1, 2 * W - 1) if op == 's2_fwd_odd' else (2 * H, 2 * W))
    x, w, bias = _rnd(1, B, Cin, Hs, Ws), _rnd(2, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5, _rnd(3, Cout)
    xr = x.double().requires_grad_(True)
    conv = F.conv2d(F.interpolate(xr, scale_factor=2, mode='nearest'), w.double(), None, padding=1) if up else \
        F.conv2d(xr, w.double(), None, stride=2, padding=1)
    if op.endswith('dgrad'):
        gy, res = _rnd(5, *conv.shape), _rnd(4, *x.shape)
        out, = torch.autograd.grad(conv, xr, gy.double())
    else:
        gy, res, out = None, _rnd(4, *conv.shape), conv.detach()
    return x, w, bias, res, gy, out


@pytest.mark.parametrize('extras', [True, False], ids=['bias_res', 'plain'])
@pytest.mark.parametrize('op,case', PARAMS, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_conv_resample_f32(op, case, extras):
    x, w, bias, res, gy, ref = _reference(op, case)
    B, Cin, Cout = x.shape[0], x.shape[1], w.shape[0]
    mode = ops.UP2 if op.startswith('up2') else ops.S2
    code = {'s2_fwd': ops.RS_S2_FWD, 's2_fwd_odd': ops.RS_S2_FWD, 's2_dgrad': ops.RS_S2_DGRAD, 'up2_fwd': ops.RS_UP2_FWD,
            'up2_dgrad': ops.RS_UP2_DGRAD}[op]
    assert ops.f32_resample_ok(B, x.shape[2], x.shape[3], Cin, Cout, code)
    dev = lambda t: t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()   # noqa: E731
    wf, wd = ops.pack_weight(w.cuda(), torch.float32, True, True)
    rd = dev(res) if extras else None
    if op.endswith('dgrad'):         # data-gradient ops take a residual only
        gd = dev(gy)
        run = lambda: ops.conv_dgrad_raw(gd, wd, mode, 9, x.shape, residual=rd)   # noqa: E731
        ref = ref + (res.double() if extras else 0)
    else:
        xd, bd = dev(x), (dev(bias) if extras else None)
        run = lambda: ops.conv_raw(xd, wf, bd, rd, None, None, None, 0, 0.0, mode, 9, 0, Cout)   # noqa: E731
        ref = ref + (bias.double()[None, :, None, None] + res.double() if extras else 0)
    y = run()
    assert y.shape == ref.shape
    r = _rel(y, ref)
    print(op, 'rel', r)
    assert r < TOL
    assert torch.equal(run(), y)
