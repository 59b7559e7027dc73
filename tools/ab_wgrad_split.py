"""Per-shape A/B of the split-bf16 fp32 weight gradient: ops.conv_wgrad_bias_raw with ops._F32_SPLIT_WGRAD on (new:
idf_conv_wgrad_f32_split) against off (old: idf_conv_wgrad_f32, the exact route) under bf16x3 and bf16x2 -- same process, alternating
sides, device events, >= 0.2 s per window, three windows per side; median [min..max] in us per call.  Gate: PASS when old - new
exceeds the larger min..max range of the two sides.  The stride-1 weight-gradient shapes of the B = 32 fp32 step."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infodiffusion_amd import ops  # noqa: E402

B = 32
SHAPES = [(64, 64, 64, 64, 9), (128, 64, 64, 64, 9), (64, 32, 32, 128, 9), (128, 32, 32, 128, 9), (256, 32, 32, 128, 9),
          (128, 16, 16, 256, 9), (256, 16, 16, 256, 9), (512, 16, 16, 256, 9), (256, 8, 8, 256, 9), (512, 8, 8, 256, 9),
          (128, 64, 64, 64, 1), (64, 32, 32, 128, 1), (256, 32, 32, 128, 1), (128, 16, 16, 256, 1), (256, 16, 16, 256, 1),
          (512, 16, 16, 256, 1), (512, 8, 8, 256, 1)]      # (Cin, H, W, Cout, taps)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    for Cin, H, W, Cout, taps in SHAPES:
        a = torch.randn(B, Cin, H, W, device='cuda').contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, Cout, H, W, device='cuda').contiguous(memory_format=torch.channels_last)

        def side(on):
            def fn():
                ops._F32_SPLIT_WGRAD = on
                return ops.conv_wgrad_bias_raw(a, dy, ops.S1, taps, True)
            return fn
        ops.set_f32_mfma('exact')
        exact = ops.conv_wgrad_bias_raw(a, dy, ops.S1, taps, True)[0]
        line = '%s B,Cin,H,W,Cout %d,%d,%d,%d,%d' % ('3x3' if taps == 9 else '1x1', B, Cin, H, W, Cout)
        for terms, mode in ((3, 'bf16x3'), (2, 'bf16x2')):
            ops.set_f32_mfma(mode)
            if not ops.f32_wgrad_split_ok(B, H, W, Cin, Cout, taps, terms):
                line += ' | x%d refused by the plan' % terms
                continue
            old, new = side(False), side(True)
            err = float((new()[0] - exact).abs().max() / exact.abs().max())
            for fn in (old, new):
                window(fn, 20)
            iters = max(10, int(0.2e6 / max(window(old, 20), window(new, 20))) + 1)
            to, tn = [], []
            for _ in range(3):
                to.append(window(old, iters))
                tn.append(window(new, iters))
            (mo, lo, ho), (mn, ln, hn) = stats(to), stats(tn)
            gate = 'PASS' if mo - mn > max(ho - lo, hn - ln) else 'FAIL'
            line += ' | x%d old %7.1f [%7.1f..%7.1f] new %7.1f [%7.1f..%7.1f] x%.2f %s err %.2e' % (terms, mo, lo, ho, mn, ln, hn, mo / mn, gate, err)
        ops.set_f32_mfma('exact')
        ops._F32_SPLIT_WGRAD = True
        print(line, flush=True)


if __name__ == '__main__':
    main()
