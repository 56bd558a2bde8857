"""What the stochastic broadcast fixture (broadcast_stoch_small.npz) adds to ``broadcast_cases.inputs()``, listed
once for the golden generator (make_golden_broadcast_stoch.py) and the tests (test_broadcast_stoch_golden.py,
test_gpu_channel_broadcast_stoch.py): the recorded uniforms that stand in for ``torch.rand_like``. They are not
stored (the fixture has to stay within 256 KiB): this seeded recipe reproduces them, one plane per broadcast step
and ndim > 1 tensor, shared by the six runs (three codecs, bits 8 and 4).
"""

import numpy as np

import delta_cases

RUNS = [(c, b) for c in ("qsgd", "rqsgd", "cnat") for b in (8, 4)]
CODED = [name for name, shape, _ in delta_cases.DICT_SHAPES if len(shape) > 1]


def uniforms(step: int) -> dict:
    """name -> fp32 uniforms in [0, 1) shaped like the tensor, for broadcast step 1..3."""
    out = {}
    for i, (name, shape, _) in enumerate(delta_cases.DICT_SHAPES):
        if len(shape) > 1:
            n = int(np.prod(shape))
            out[name] = np.random.default_rng(7000 + 100 * step + i).random(n, dtype=np.float32).reshape(shape)
    return out
