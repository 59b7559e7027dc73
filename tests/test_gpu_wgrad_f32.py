"""GPU: the fp32 ordered-slab weight gradient (idf_conv_wgrad_f32) through ops.conv_wgrad_bias_raw against a float64
convolution's autograd on the host, at the project's fp32 bound, and bit-identical from call to call."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL = 2e-5      # tests/test_gpu_kernels.py TOL[torch.float32]

CASES = [
    # (B, Cin, H, W, Cout, taps)
    (2, 64, 4, 4, 64, 9),           # smallest map, one tile, one split
    (3, 36, 7, 7, 20, 9),           # odd map and batch, ragged channel tiles on both sides, K-steps that wrap rows
    (2, 64, 8, 16, 64, 9), (2, 64, 16, 8, 64, 9),     # H != W, both ways
    (2, 32, 28, 28, 64, 9),         # W not a power of two
    (2, 32, 14, 14, 64, 9),         # 4-row tiles on 14 rows: the last row tile of an image masks rows
    (2, 72, 16, 16, 136, 9),        # a full plus a ragged 64-tile in both channel dimensions
    (5, 64, 32, 32, 64, 9),         # pixel splits that start and end inside an image, uneven last split
    (3, 64, 64, 64, 64, 9),         # widest map, one channel tile pair, the most slabs
    (2, 256, 8, 8, 256, 9),         # many channel tiles, few pixels
    (2, 64, 16, 16, 72, 1), (3, 256, 16, 16, 256, 1), (2, 64, 64, 64, 64, 1),     # 1x1: ragged cout, many tiles, many splits
]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_wgrad_f32(case):
    B, Cin, H, W, Cout, taps = case
    k = 3 if taps == 9 else 1
    a, dy = _rnd(1, B, Cin, H, W), _rnd(2, B, Cout, H, W)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    gw, gb = torch.autograd.grad(F.conv2d(a.double(), w, b, padding=k // 2), (w, b), dy.double())

    assert ops.f32_wgrad_ok(B, H, W, Cin, Cout, taps)
    ad, dyd = a.cuda().contiguous(memory_format=CL), dy.cuda().contiguous(memory_format=CL)
    dW, db = ops.conv_wgrad_bias_raw(ad, dyd, ops.S1, taps, True)
    assert dW.shape == gw.shape and db.shape == gb.shape
    rw, rb = _rel(dW, gw), _rel(db, gb)
    print('dW rel', rw, 'db rel', rb)
    assert rw < TOL and rb < TOL
    dW2, db2 = ops.conv_wgrad_bias_raw(ad, dyd, ops.S1, taps, True)
    assert torch.equal(dW2, dW) and torch.equal(db2, db)


def test_wgrad_f32_without_bias():
    B, Cin, H, W, Cout, taps = CASES[4]         # several slabs: the reduce stops in front of db
    ad, dyd = (_rnd(s, B, C, H, W).cuda().contiguous(memory_format=CL) for s, C in ((1, Cin), (2, Cout)))
    dW, db = ops.conv_wgrad_bias_raw(ad, dyd, ops.S1, taps, False)
    assert db is None and torch.equal(dW, ops.conv_wgrad_bias_raw(ad, dyd, ops.S1, taps, True)[0])
