"""Host restatement of the counter-based dropout masks of the fused ``leaky_relu + dropout`` epilogues.

TEST INFRASTRUCTURE (see ``oracle/__init__.py``).  Written from the contract in ``include/qot_gnn.h`` ("keep =
hash(seed, *step_counter, element) >= p") and the arithmetic it stands for; numpy ``uint64`` and torch on the CPU only, no
code shared with ``gnn_qot_estimation_amd``.  The masks are no random stream: they are a pure function of ``(seed, step,
flat element index)``, so the fp64 oracle can run the very dropout realisation a HIP train step ran.

The rule:

* elements are numbered row-major over the activation's shape (``flat``);
* one 64-bit hash serves four consecutive elements (``idx4 = flat >> 2``); element ``c = flat & 3`` draws bits
  ``16c .. 16c + 15`` of it;
* ``keep = draw >= thr16`` with ``thr16 = min(floor(float32(p) * 65536 + 0.5), 65535)`` in fp32 arithmetic; ``thr16 == 0``
  keeps everything;
* kept values are scaled by ``float32(1) / (float32(1) - float32(p))``;
* the hash: ``k = seed ^ (step * 0x9E3779B97F4A7C15 mod 2^64)``, split into 32-bit halves ``k0`` (low) and ``k1``; three
  32 x 32 -> 64 multiplies, each folded ``hi ^ lo``.
"""
from __future__ import annotations

import numpy as np
import torch

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HEAD_SITE = 97          # the read-out head's multiplier; convolution l (1-based) uses l


def thr16(p: float) -> int:
    """The 16-bit keep threshold of probability ``p``, rounded as fp32 arithmetic rounds it."""
    p32 = np.float32(p)
    if not p32 > 0:
        return 0
    t = int(np.float32(p32 * np.float32(65536.0)) + np.float32(0.5))
    return min(t, 65535)


def keep_scale(p: float) -> np.float32:
    """``1 / (1 - p)`` evaluated in fp32, the factor a kept element is multiplied by."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def site_seed(base_seed: int, site) -> int:
    """Seed of one dropout site of ``TopologicalGNN``: ``site`` is ``"conv<l>"`` (or the 1-based integer ``l``) for the
    activation after convolution ``l``, ``"head"`` for the dropout inside the read-out MLP."""
    if site == "head":
        mult = HEAD_SITE
    elif isinstance(site, str):
        if not site.startswith("conv"):
            raise ValueError(site)
        mult = int(site[4:])
    else:
        mult = int(site)
    if mult < 1:
        raise ValueError(site)
    return (int(base_seed) + GOLDEN * mult) & MASK64


def _hash64(seed: int, step: int, idx4: np.ndarray) -> np.ndarray:
    k = (int(seed) & MASK64) ^ ((int(step) * GOLDEN) & MASK64)
    k0, k1 = np.uint64(k & 0xFFFFFFFF), np.uint64(k >> 32)
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    lo = idx4 & m32
    hi = idx4 >> s32
    p = (lo ^ k0) * np.uint64(0x9E3779B1)                     # 32 x 32: no overflow in uint64
    a = ((p >> s32) ^ (p & m32) ^ hi ^ k1) & m32
    q = a * np.uint64(0x85EBCA77)
    r = ((a ^ k0 ^ np.uint64(0x68E31DA4)) & m32) * np.uint64(0xC2B2AE3D)
    w0 = ((q >> s32) ^ q) & m32
    w1 = ((r >> s32) ^ r) & m32
    return (w1 << s32) | w0


def keep_mask(seed: int, step: int, shape, p: float) -> torch.Tensor:
    """Bool tensor of ``shape``: True where the element of that row-major index is kept at ``(seed, step)``."""
    shape = tuple(int(s) for s in (shape if hasattr(shape, "__iter__") else (shape,)))
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    t = thr16(p)
    if t == 0 or n == 0:
        return torch.ones(shape, dtype=torch.bool)
    flat = np.arange(n, dtype=np.uint64)
    z = _hash64(seed, step, flat >> np.uint64(2))
    draw = (z >> (np.uint64(16) * (flat & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.from_numpy(draw >= np.uint64(t)).reshape(shape)


KERNEL_WIDTHS = (16, 32, 64, 128, 256)


def indexed_width(width: int) -> int:
    """The width the elements of a ``[rows, width]`` activation are numbered at: the kernels exist for ``KERNEL_WIDTHS``
    and any other width runs zero-padded to the next of them."""
    for w in KERNEL_WIDTHS:
        if width <= w:
            return w
    raise ValueError(width)


def topological_masks(base_seed: int, step: int, p: float, num_nodes: int, num_graphs: int, width: int,
                      num_layers: int = 2, head: bool = True):
    """``{site: keep}`` of one train-mode forward of ``TopologicalGNN``: ``[num_nodes, width]`` after every convolution and
    ``[num_graphs, width]`` inside the read-out (``head=False``: without it, for a read-out that runs torch's own
    ``nn.Dropout``).  A width that runs zero-padded is numbered at the padded width; the masks returned are its first
    ``width`` columns."""
    w = indexed_width(width)
    keep = {f"conv{l}": keep_mask(site_seed(base_seed, l), step, (num_nodes, w), p)[:, :width]
            for l in range(1, num_layers + 1)}
    if head:
        keep["head"] = keep_mask(site_seed(base_seed, "head"), step, (num_graphs, w), p)[:, :width]
    return keep
