"""Microscaling (MX) fake-quantizer: blocks of 32 elements under one E8M0 power-of-two scale byte, elements in OCP E4M3FN,
E5M2, the 6-bit E2M3 / E3M2 or the 4-bit E2M1 -- the operands of the MI355X's scaled matrix instructions, held by
torch.float8_e8m0fnu and torch.float4_e2m1fn_x2.  torch has no 6-bit dtype: fmt="e2m3" / "e3m2" name those formats, their
codes are torch.uint8 [..., 3K / 4] (four elements in three bytes), and the row length K must be a multiple of 4.

    forward(x) = decode(encode(x))      on the kernels of csrc/fp8q_mx.hip (include/fp8q.h states the arithmetic)

The scale of a block is a function of that block's own largest element, found inside the quantizing pass: there is no range
to estimate, calibrate, fix or learn.  `range_free = True` tells QuantizationManager so -- it calls the quantizer directly in
every state and never runs its estimator.  Blocks run along the last dimension, the reduction dimension of a Linear weight
[out, in] and of its input; flatten_rows=True views a tensor of more than two dimensions as [shape[0], -1] first, which is
what a convolution weight [out, in, kh, kw] wants.  block_axis=-2 runs the blocks along dim 0 of that 2-D view instead
(csrc/fp8q_mx_t.hip): the operand of a product that reduces over dim 0 -- dx = dy . W over W's rows, dW = dy^T . x over the
tokens -- whose blocks hold other elements than the row-wise ones, so its scales and rounding differ.  encode() then returns
the operands of the transpose, [K, R]-shaped, and the tensor must be 2-D after flatten_rows and as divisible along dim 0 as
the format's packing asks (E2M1: even, the 6-bit formats: a multiple of 4).

stochastic=True rounds the elements stochastically instead of to nearest even (include/fp8q.h: 16 bits of Philox4x32-10 per
element), which is what the operands of a backward product want: call number n of forward / encode uses the seed
(seed + n) mod 2^64 and records it as `last_seed`, so that ops.mx_quantize(x, ..., seed=q.last_seed) reproduces the call;
reseed(seed) starts the count again.

It follows the quantizer protocol (QuantizerBase) and the model zoo takes it as `method=MXQuantizer`; it is deliberately NOT a
member of QMethods (the CLI's choices).  Forward only: there is no backward kernel, and a call that would need a gradient
raises NotImplementedError.  There is no CPU path.
"""
import torch

from fp8q import ops as _ops
from .fp8 import QuantizerBase

_HALF = (torch.float16, torch.bfloat16)
_BITS = {torch.float8_e4m3fn: 8, torch.float8_e5m2: 8, torch.float4_e2m1fn_x2: 4, _ops.MX_E2M3: 6, _ops.MX_E3M2: 6}
_NAME = {torch.float8_e4m3fn: "E4M3FN", torch.float8_e5m2: "E5M2", torch.float4_e2m1fn_x2: "E2M1", _ops.MX_E2M3: "E2M3",
         _ops.MX_E3M2: "E3M2"}


class MXQuantizer(QuantizerBase):
    range_free = True

    def __init__(self, n_bits=None, fmt=torch.float8_e4m3fn, rounding="floor", keep_dtype=False, flatten_rows=False,
                 per_channel=False, scale_domain=None, block_axis=-1, stochastic=False, seed=0, **kwargs):
        if not isinstance(fmt, (torch.dtype, str)) or fmt not in _BITS:
            raise ValueError(f"fmt must be torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, 'e2m3' or 'e3m2', "
                             f"got {fmt!r}")
        if n_bits is not None and n_bits != _BITS[fmt]:
            raise ValueError(f"{_NAME[fmt]} elements have {_BITS[fmt]} bits, got n_bits={n_bits}")
        if rounding not in ("floor", "ceil"):
            raise ValueError(f"rounding must be 'floor' or 'ceil', got {rounding!r}")
        if block_axis not in (-1, -2) or isinstance(block_axis, bool):
            raise ValueError(f"block_axis must be -1 (blocks along the last dimension) or -2 (along dim 0 of the 2-D view), "
                             f"got {block_axis!r}")
        if not isinstance(stochastic, bool):
            raise ValueError(f"stochastic must be True or False, got {stochastic!r}")
        self._check_seed(seed)
        # per_channel is the protocol's argument; the scales are per block either way
        super().__init__(n_bits=_BITS[fmt], per_channel=per_channel, **kwargs)
        self.fmt = fmt
        self.rounding = rounding
        # float16 / bfloat16 inputs: False returns float32, True the input's dtype (the float32 value rounded once)
        self.keep_dtype = keep_dtype
        self.flatten_rows = flatten_rows
        self.block_axis = block_axis
        self.stochastic = stochastic
        self.reseed(seed)

    @staticmethod
    def _check_seed(seed):
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be a Python int in [0, 2^64), got {seed!r}")

    def reseed(self, seed):
        """start again from `seed`: the next stochastic call uses it, the one after seed + 1, ..."""
        self._check_seed(seed)
        self.seed = seed
        self.calls = 0
        self.last_seed = None

    def _draw(self):
        """the keywords this call adds to its op: none unless stochastic, else seed=(seed + calls) mod 2^64, recorded as
        last_seed"""
        if not self.stochastic:
            return {}
        self.last_seed = (self.seed + self.calls) % (1 << 64)
        self.calls += 1
        return {"seed": self.last_seed}

    @property
    def is_initialized(self):
        return True

    @property
    def symmetric(self):
        return True

    def reset(self):
        pass

    def set_quant_range(self, x_min, x_max):
        pass

    def fix_ranges(self):
        pass

    def make_range_trainable(self):
        raise NotImplementedError("MXQuantizer is forward-only and has no range: nothing can be learned")

    def _rows(self, t):
        """t as the kernels cut it into blocks: along the last dimension, of [shape[0], -1] with flatten_rows"""
        if self.flatten_rows and t.dim() > 2:
            return t.contiguous().view(t.shape[0], -1)
        return t

    def _matrix(self, t):
        """_rows(t) for block_axis=-2: it must be a matrix whose transposed operands can be made (ops.mx_encode_t's rules),
        so that decode(*encode(x)) == forward(x) holds for every tensor forward takes"""
        t = self._rows(t)
        _ops._mx_t_geometry(t, self.fmt)
        return t

    def forward(self, x_float):
        if torch.is_grad_enabled() and x_float.requires_grad:
            raise NotImplementedError("MXQuantizer is forward-only: there is no backward kernel for the MX lane (call it "
                                      "under torch.no_grad(), or on a detached tensor)")
        out_dtype = x_float.dtype if (self.keep_dtype and x_float.dtype in _HALF) else None
        if self.block_axis == -2:
            t, op = self._matrix(x_float), _ops.mx_quantize_t
        else:
            t, op = self._rows(x_float), _ops.mx_quantize
        y = op(t, self.fmt, self.rounding, out_dtype=out_dtype, **self._draw())
        return y.view(x_float.shape)

    def encode(self, x_float):
        """(codes, scales) of forward(x): codes of dtype `fmt` ([..., K] for FP8, [..., K / 2] for E2M1; torch.uint8
        [..., 3K / 4] for the 6-bit formats), scales torch.float8_e8m0fnu [..., ceil(K / 32)]; with flatten_rows, of the
        [shape[0], -1] view.  block_axis=-2: the operands of that view's transpose, ops.mx_encode_t's."""
        if self.block_axis == -2:
            t, op = self._matrix(x_float.detach()), _ops.mx_encode_t
        else:
            t, op = self._rows(x_float.detach()), _ops.mx_encode
        return op(t, self.fmt, self.rounding, **self._draw())

    def decode(self, codes, scales, out_dtype=None):
        """Values of encode()'s operands, float32 or out_dtype (float16 / bfloat16: the float32 value rounded once), shaped as
        encode() saw them: decode(*encode(x)) == forward(x) bit for bit (after .view(x.shape) with flatten_rows).
        block_axis=-2: the transposed operands decode to [K, R]; the result is that, transposed back (a view)."""
        if self.block_axis == -2:
            return _ops.mx_decode(codes, scales, fmt=self.fmt, out_dtype=out_dtype).t()
        return _ops.mx_decode(codes, scales, fmt=self.fmt, out_dtype=out_dtype)

    def extra_repr(self):
        sr = f"stochastic=True, seed={self.seed}, " if self.stochastic else ""
        return f"{super().extra_repr()}, fmt={_NAME[self.fmt]}, rounding={self.rounding}, flatten_rows={self.flatten_rows}, " \
               f"{sr}block_axis={self.block_axis}"
