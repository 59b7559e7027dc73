"""GPU: the split-bf16 3x3 conv (idf_conv3x3_f32_split, modes bf16x3 / bf16x2 of ops.set_f32_mfma) through ops.conv_raw /
ops.conv_dgrad_raw against a float64 convolution on the host.  Bounds are derived, not measured: bf16x3 drops < 3 * 2^-27 per
product and is held to the project's fp32 bound; a two-term residual is <= 2^-18 relative per operand, so bf16x2 is held
elementwise to 3 * 2^-18 * conv(|x|, |w|) plus the fp32 bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from infodiffusion_amd import ops  # noqa: E402

CL = torch.channels_last
TOL = 2e-5              # tests/test_gpu_kernels.py TOL[torch.float32]
TOL2 = 3 * 2.0 ** -18   # bf16x2, per product magnitude
MODE = {3: 'bf16x3', 2: 'bf16x2'}

CASES = [
    # (B, Cin, H, W, Cout)
    (2, 32, 4, 4, 64),          # one chunk, smallest map
    (2, 64, 8, 16, 64), (2, 64, 16, 8, 64),     # H != W, both ways
    (3, 32, 7, 7, 32),          # odd map and batch
    (2, 32, 28, 28, 64),        # W not a power of two
    (2, 64, 16, 16, 72),        # full plus ragged cout tile
    (2, 64, 16, 16, 3),         # one ragged tile
    (2, 192, 8, 8, 64),         # 6 chunks, buffer parity
    (2, 32, 10, 20, 32),        # last row tile masks rows
    (3, 64, 64, 64, 64),        # many row tiles
    (32, 32, 64, 64, 64),       # chip-filling grid: the largest tile form
]


def _rnd(seed, *shape):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _dev(t):
    return t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()


def _convs(x, w, gy):
    """float64 conv and data gradient, and the same of the magnitudes."""
    xr = x.double().requires_grad_(True)
    conv = F.conv2d(xr, w.double(), None, padding=1)
    gx, = torch.autograd.grad(conv, xr, gy.double())
    gxm, = torch.autograd.grad(F.conv2d(xr, w.double().abs(), None, padding=1), xr, gy.double().abs())
    return conv.detach(), gx, F.conv2d(x.double().abs(), w.double().abs(), None, padding=1), gxm


@functools.lru_cache(maxsize=2)
def _reference(case):
    B, Cin, H, W, Cout = case
    x, w = _rnd(1, B, Cin, H, W), _rnd(2, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5
    bias, res, gy = _rnd(3, Cout), _rnd(4, B, Cout, H, W), _rnd(5, B, Cout, H, W)
    return (x, w, bias, res, gy) + _convs(x, w, gy)


def _check(tag, terms, y, ref, mag):
    err = (y.detach().cpu().double() - ref).abs()
    peak = float(ref.abs().max())
    print(tag, 'terms', terms, 'rel', float(err.max()) / peak, 'of elementwise bound', float((err / (TOL2 * mag + TOL * peak)).max()))
    if terms == 3:
        assert float(err.max()) / peak < TOL
    else:
        assert bool((err <= TOL2 * mag + TOL * peak).all())


@pytest.fixture
def mfma_mode():
    yield ops.set_f32_mfma
    ops.set_f32_mfma('exact')


def _run(mfma_mode, terms, x, w, bias, res, gy):
    """(y, dx) under the split mode, after the checks that do not need a reference."""
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    wf, wd = ops.pack_weight(w.cuda(), torch.float32, True, True)
    xd, bd, rd = _dev(x), (_dev(bias) if bias is not None else None), (_dev(res) if res is not None else None)
    args = (xd, wf, bd, rd, None, None, None, 0, 0.0, ops.S1, 9, 0, Cout)
    assert ops.f32_split_ok(B, H, W, Cin, Cout, terms)     # (the data gradient of a Cout that is no multiple of 32 stays exact)
    # mode 'exact' is the halo kernel's launch, bit for bit
    halo = ops.empty_nhwc(B, Cout, H, W, torch.float32, xd.device)
    ops.call('idf_conv3x3_f32', ops._p(xd), ops._p(wf), ops._p(bd), ops._p(rd), ops._p(halo), B, H, W, Cin, Cout, ops._st())
    assert ops.get_f32_mfma() == 'exact' and torch.equal(ops.conv_raw(*args), halo)
    mfma_mode(MODE[terms])
    y = ops.conv_raw(*args)
    assert not torch.equal(y, halo) and torch.equal(ops.conv_raw(*args), y)
    dx = ops.conv_dgrad_raw(_dev(gy), wd, ops.S1, 9, x.shape)
    return y, dx


@pytest.mark.parametrize('terms', [3, 2])
@pytest.mark.parametrize('extras', [True, False], ids=['bias_res', 'plain'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_split_fwd_dgrad(case, extras, terms, mfma_mode):
    x, w, bias, res, gy, conv, gx, mag, gxm = _reference(case)
    y, dx = _run(mfma_mode, terms, x, w, bias if extras else None, res if extras else None, gy)
    add = bias.double()[None, :, None, None] + res.double() if extras else torch.zeros(())
    assert y.shape == conv.shape
    _check('fwd', terms, y, conv + add, mag + add.abs())
    _check('dgrad', terms, dx, gx, gxm)


def _emulate(a, w, terms):
    """The kernel's arithmetic on the host: bf16 terms by torch's round-to-nearest-even, the kept products summed in float64."""
    def split(v):
        out, r = [], v.clone()
        for _ in range(terms):
            out.append(r.bfloat16().float())
            r = r - out[-1]
        return [t.double() for t in out]
    at, wt = split(a), split(w)
    keep = [(0, 0), (0, 1), (1, 0)] + ([(1, 1), (0, 2), (2, 0)] if terms == 3 else [])
    return sum(F.conv2d(at[i], wt[j], None, padding=1) for i, j in keep)


@pytest.mark.parametrize('terms', [3, 2])
def test_conv3x3_split_scales(terms, mfma_mode):
    """The tail conv's gain on the weights and 2^-20 .. 2^20 across the channels of x: the bounds are scale-aware."""
    B, Cin, H, W, Cout = 2, 64, 16, 16, 64
    k = torch.arange(Cin) % 41 - 20
    x = _rnd(11, B, Cin, H, W) * (2.0 ** k.double()).float()[None, :, None, None]
    w = _rnd(12, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5 * 1e-5
    bias, res, gy = _rnd(13, Cout) * 1e-5, _rnd(14, B, Cout, H, W), _rnd(15, B, Cout, H, W)
    conv, gx, mag, gxm = _convs(x, w, gy)
    add = bias.double()[None, :, None, None] + res.double()
    # the emulation itself meets the bound (fp32 accumulation aside), so the bound is a fair one for the kernel
    _check('emulated', terms, _emulate(x, w, terms), conv, mag)
    y, dx = _run(mfma_mode, terms, x, w, bias, res, gy)
    _check('fwd', terms, y, conv + add, mag + add.abs())
    _check('dgrad', terms, dx, gx, gxm)
    wf, _ = ops.pack_weight(w.cuda(), torch.float32, True, True)
    y0 = ops.conv_raw(torch.zeros_like(_dev(x)), wf, _dev(bias), _dev(res), None, None, None, 0, 0.0, ops.S1, 9, 0, Cout)
    assert torch.equal(y0, _dev(res) + _dev(bias)[None, :, None, None])
