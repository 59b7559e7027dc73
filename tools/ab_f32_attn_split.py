"""Per-shape A/B of the split-bf16 fp32 attention: python tools/ab_f32_attn_split.py [MODE ...]   (default: bf16x3 bf16x2)
One process, alternating sides, device events.  new = ops._F32_SPLIT_ATTN True, old = False (the routing of 'exact' mode).  Per
row: warm-up of both sides, iteration count for >= 0.2 s per window sized by the old side, 3 windows per side alternating; median
and [min..max] in us per call (allocation and autograd included on both sides).  gate = old - new > the larger [min..max] range of
the two sides.  The rows are those of profiles/f32_attn.txt section 1."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from infodiffusion_amd import ops  # noqa: E402

ROWS = [(32, 256, 128), (32, 64, 128), (32, 256, 64), (32, 64, 64), (256, 256, 128), (256, 64, 128)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    modes = sys.argv[1:] or ['bf16x3', 'bf16x2']
    print('mode,B,N,D,what            new_us   new[min..max]     old_us   old[min..max]   speedup gate  maxdiff')
    for mode in modes:
        ops.set_f32_mfma(mode)
        for B, N, D in ROWS:
            H = int(N ** 0.5)
            g = torch.Generator(device='cpu').manual_seed(1)
            qkv = torch.randn(B, 3 * D, H, H, generator=g).cuda().contiguous(memory_format=torch.channels_last)
            do = torch.randn(B, D, H, H, generator=g).cuda().contiguous(memory_format=torch.channels_last)
            qg = qkv.clone().requires_grad_(True)

            def fwd():
                with torch.no_grad():
                    return ops.attention(qkv)

            def both():
                return torch.autograd.grad(ops.attention(qg), qg, do)[0]

            for what, fn in (('fwd', fwd), ('fwd+bwd', both)):
                res = {}
                for side in (True, False):
                    ops._F32_SPLIT_ATTN = side
                    res[side] = fn().clone()
                    window(fn, 20)
                iters = max(10, int(0.2e6 / window(fn, 50)))          # the old side is set
                t = {True: [], False: []}
                for _ in range(3):
                    for side in (True, False):
                        ops._F32_SPLIT_ATTN = side
                        t[side].append(window(fn, iters))
                ops._F32_SPLIT_ATTN = True
                new, old = statistics.median(t[True]), statistics.median(t[False])
                spread = max(max(t[True]) - min(t[True]), max(t[False]) - min(t[False]))
                diff = float((res[True] - res[False]).abs().max() / res[False].abs().max())
                print('%s,%d,%d,%d,%-8s %8.1f %8.1f..%-8.1f %8.1f %8.1f..%-8.1f %6.2f  %s %.2e' % (
                    mode, B, N, D, what, new, min(t[True]), max(t[True]), old, min(t[False]), max(t[False]), old / new,
                    'ok  ' if old - new > spread else 'FAIL', diff), flush=True)
    ops.set_f32_mfma('exact')


if __name__ == '__main__':
    main()
