"""The inputs of the broadcast fixture (broadcast_small.npz), listed once: the golden generator
(make_golden_broadcast.py) and the tests (test_broadcast_golden.py, test_gpu_channel_broadcast.py) take them from
here. Three successive broadcasts over ``delta_cases.dict_pair()``: the hidden state starts as prev, g of step 1
is new, and g moves again before steps 2 and 3. The tensors above SHA_ABOVE elements are not stored in the
fixture (it has to stay within 256 KiB): this recipe reproduces them, and the fixture pins their SHA-256.
"""

import hashlib

import numpy as np

import delta_cases

STEPS = 3
SHA_ABOVE = 4096      # larger tensors: the fixture holds a SHA-256 of the bytes instead of the array
FROZEN = "fc.weight"  # in step 3, g's tensor is exactly the hidden state (it depends on bits: stored)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def moved(g: dict, step: int) -> dict:
    """g of the next step: every float entry moves again (grid data stays grid data), the counter counts on."""
    out = {}
    for i, (name, a) in enumerate(g.items()):
        if a.dtype == np.int64:
            out[name] = np.array(a + 3, dtype=np.int64)
        elif a.size > SHA_ABOVE:
            d = delta_cases.grid(a.size, 1000 * step + i, 8, 2.0 ** -9).reshape(a.shape)
            out[name] = (a + d).astype(np.float32)
        else:
            rng = np.random.default_rng(2000 * step + i)
            out[name] = (a + np.float32(2e-3) * rng.standard_normal(a.shape, dtype=np.float32)).astype(np.float32)
    return out


def inputs():
    """(h0, [g of step 1, 2, 3]) as name -> numpy array dicts in DICT_SHAPES order. Step 3's FROZEN entry is a
    placeholder: the caller replaces it with the hidden state it has reached."""
    prev, new = delta_cases.dict_pair()
    news = [new]
    for k in range(2, STEPS + 1):
        news.append(moved(news[-1], k))
    return prev, news
