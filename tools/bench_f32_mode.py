"""Run bench.py unchanged under an fp32 arithmetic mode: python tools/bench_f32_mode.py MODE WGRAD [ATTN] [bench.py arguments]
MODE = exact | bf16x3 | bf16x2 (ops.set_f32_mfma), WGRAD = 1 | 0 (ops._F32_SPLIT_WGRAD: 0 keeps the weight gradients exact),
ATTN = 1 (default) | 0 (ops._F32_SPLIT_ATTN: 0 keeps the attention on the routes of 'exact' mode)."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from infodiffusion_amd import ops  # noqa: E402

if __name__ == '__main__':
    mode, wgrad = sys.argv[1], sys.argv[2]
    ops.set_f32_mfma(mode)
    ops._F32_SPLIT_WGRAD = wgrad == '1'
    rest = sys.argv[3:]
    if rest and rest[0] in ('0', '1'):
        ops._F32_SPLIT_ATTN = rest.pop(0) == '1'
    sys.argv = [os.path.join(ROOT, 'bench.py')] + rest
    runpy.run_path(sys.argv[0], run_name='__main__')
