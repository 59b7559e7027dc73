"""GPU: the fp32 halo-tile 3x3 conv (idf_conv3x3_f32) through ops.conv_raw / ops.conv_dgrad_raw against a float64
convolution on the host, at the project's fp32 bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL = 2e-5      # tests/test_gpu_kernels.py TOL[torch.float32]

CASES = [
    # (B, Cin, H, W, Cout)
    (2, 32, 4, 4, 64),          # smallest map, one K chunk pair
    (2, 64, 8, 16, 64), (2, 64, 16, 8, 64),     # H != W, both ways
    (3, 32, 7, 7, 32),          # odd map, odd batch
    (2, 32, 28, 28, 64),        # W not a power of two
    (2, 64, 16, 16, 3),         # one ragged cout tile
    (2, 64, 16, 16, 72),        # full tile plus ragged tile
    (2, 192, 8, 8, 64),         # 12 chunks, ring parity
    (3, 64, 64, 64, 64),        # many row tiles per image, widest map, odd batch (128-pixel tiles)
    (2, 256, 32, 32, 128),      # two cout tiles, longest K
    (2, 32, 10, 20, 32),        # 3-row tiles: the last tile of an image masks rows
    (32, 32, 64, 64, 64),       # a grid that fills the chip: the 256-pixel tiles
    (3, 32, 64, 64, 3), (32, 32, 64, 64, 3),    # the 16-wide cout tile at 128- and 256-pixel tiles
]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=2)
def _reference(case):
    B, Cin, H, W, Cout = case
    x, w = _rnd(1, B, Cin, H, W), _rnd(2, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5
    bias, res, gy = _rnd(3, Cout), _rnd(4, B, Cout, H, W), _rnd(5, B, Cout, H, W)
    xr = x.double().requires_grad_(True)
    conv = F.conv2d(xr, w.double(), None, padding=1)
    gx, = torch.autograd.grad(conv, xr, gy.double())
    return x, w, bias, res, gy, conv.detach(), gx


@pytest.mark.parametrize('extras', [True, False], ids=['bias_res', 'plain'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_f32_fwd_dgrad(case, extras):
    B, Cin, H, W, Cout = case
    x, w, bias, res, gy, conv, gx = _reference(case)
    assert ops.f32_halo_ok(B, H, W, Cin, Cout)
    dev = lambda t: t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()   # noqa: E731
    wf, wd = ops.pack_weight(w.cuda(), torch.float32, True, True)
    xd, bd, rd = dev(x), (dev(bias) if extras else None), (dev(res) if extras else None)
    y = ops.conv_raw(xd, wf, bd, rd, None, None, None, 0, 0.0, ops.S1, 9, 0, Cout)
    ref = conv + (bias.double()[None, :, None, None] + res.double() if extras else 0)
    assert y.shape == ref.shape
    r = _rel(y, ref)
    print('fwd rel', r)
    assert r < TOL
    assert torch.equal(ops.conv_raw(xd, wf, bd, rd, None, None, None, 0, 0.0, ops.S1, 9, 0, Cout), y)
    dx = ops.conv_dgrad_raw(dev(gy), wd, ops.S1, 9, x.shape)
    r = _rel(dx, gx)
    print('dgrad rel', r)
    assert r < TOL
