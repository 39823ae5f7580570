"""Shared builders of the multi-tensor launches' tests (tests/test_multi_routes.py): the tensors of a launch, their data and
ranges, the probes planted in every tensor, and the batching rules of csrc/fp8q_multi.hip:plan_build written out as literals.
A helper, not a test module; numpy only, needs no GPU.

  spec      T(shape, fmt, per_tensor, xoff, yoff): one tensor of a launch.  fmt = (mbits, n_bits, sign_bits); per_tensor: one
            range for the whole tensor instead of one per row of dim 0; xoff / yoff: bytes by which the input / the output
            pointer misses its 16-byte boundary (the float side: 0 or 4; the code side, one byte per element: 0 .. 3).
  data      make(spec, i, rng): tensor i of a launch gets normals of its own scale, 0.02 * 1.9^(i mod 12), and ranges of
            0.6 .. 2.6 times that scale (so some elements clamp), each row its own; PROBES of row 0's range are laid over
            the first elements.  A block of the batched kernel that picked a neighbour's descriptor then quantizes with a
            range several binades off, and usually another format: wrong bits, not plausible ones.
  rules     a per-channel tensor is batched when (inner + 4097) / inner + 1 table rows of 32 + (2^E + 1) * 8 bytes fit 36 KiB
            (ROW_TABLE_EDGES: the longest row that falls back and the shortest that batches, per format), 4 <= inner <= 60000,
            4 <= elements < 2^31, less than 64 MiB, and both pointers aligned for the mode.
  rowmax    rowmax_loop(p, inner): which loop of k_multi_rowmax reads element p of a row -- "main", four loads in flight per
            lane while i + 192 < inner, or "rem", one load per pass.
"""
from collections import namedtuple

import numpy as np

MODES = {0: "quantize", 3: "encode", 4: "decode"}

T = namedtuple("T", "shape fmt per_tensor xoff yoff")
T.__new__.__defaults__ = ((3, 8, 1), False, 0, 0)

# (format, longest row that falls back, shortest row that batches, modes): per-channel [16, inner].  E = n_bits - sign - M;
# (7,8,1) has no exponent bit, hence no storage codes.
ROW_TABLE_EDGES = [
    ((2, 8, 1), 33, 34, (0, 3, 4)),
    ((3, 8, 1), 18, 19, (0, 3, 4)),
    ((4, 8, 1), 11, 12, (0, 3, 4)),
    ((6, 8, 1), 6, 7, (0, 3, 4)),
    ((7, 8, 1), 5, 6, (0,)),
    ((1, 8, 0), 124, 125, (0, 3, 4)),
]

# 4096 k + t and 4096 k + 4 + t elements, k = 1, 2, t = 0 .. 3, as [C, inner] with inner a divisor (4099 is prime: [1, 4099],
# which the plan treats as one row under one range)
CHUNK_EDGE_SHAPES = [
    (64, 64), (17, 241), (6, 683), (1, 4099), (41, 100), (3, 1367), (14, 293), (11, 373),
    (128, 64), (3, 2731), (34, 241), (55, 149), (12, 683), (7, 1171), (2, 4099), (9, 911),
]
assert sorted(c * n for c, n in CHUNK_EDGE_SHAPES) == [4096 * k + a + t for k in (1, 2) for a in (0, 4) for t in range(4)]

# the (M, sign_bits, maxval) of tests/test_codes.py::test_oracle_roundtrip_equals_quantize / test_hip_codec_per_tensor, where
# decode(encode(x)) == quantize(x) bit for bit (elsewhere a binade top may come back a few ULP off: include/fp8q.h)
ROUNDTRIP_FORMATS = [(2, 1, 57344.0), (3, 1, 240.0), (3, 1, 0.7361), (5, 1, 3.0), (3, 0, 2.5), (1, 0, 0.31), (6, 1, 1.0),
                     (7, 0, 1.0)]


def probes(mv):
    mv = np.float32(mv)
    with np.errstate(over="ignore"):
        return np.array([0.0, -0.0, mv, -mv, np.float32(3) * mv, 1e-41, np.inf, -np.inf], np.float32)


def scale_of(i):
    return np.float32(0.02 * 1.9 ** (i % 12))


def make(spec, i, rng, with_probes=True):
    """(x, maxval) of tensor i of a launch, float32"""
    shape = tuple(spec.shape)
    s = scale_of(i)
    x = (rng.standard_normal(shape) * s).astype(np.float32)
    C = 1 if spec.per_tensor else shape[0]
    mv = (rng.uniform(0.6, 2.6, C) * s).astype(np.float32)
    if with_probes and x.size:
        p = probes(mv[0])
        k = min(p.size, x.size)
        x.reshape(-1)[:k] = p[:k]
    return x, mv


def rowmax_loop(p, inner):
    lane, j = p % 64, p // 64
    i = lane + 256 * (j // 4)
    return "main" if i + 192 < inner else "rem"


def rowmax_positions(inner):
    """one element index read by each loop of k_multi_rowmax, None where the row never enters that loop: the last such
    element, so that a long row's planted value sits in a late pass"""
    pos = {"main": None, "rem": None}
    for p in range(inner):
        pos[rowmax_loop(p, inner)] = p
    return pos
