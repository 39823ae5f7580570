"""Hardware FP8 fake-quantizer: the OCP encodings the MI355X's matrix cores and torch.float8_e4m3fn / torch.float8_e5m2 read.

FPQuantizer computes the reference's emulated formats (a real-valued exponent bias, no NaN or infinity codes); its storage
codes cannot be read as hardware FP8.  OCPFP8Quantizer is the other kind: a fixed format (E4M3FN, fmax 448, or E5M2, fmax
57344) under a float32 scale = max(maxval, eps) / fmax per tensor or per output channel, with
    forward(x) = decode(encode(x)),  encode(x) = RNE(clamp(x / scale, -fmax, fmax)) as OCP bytes,  decode(c) = value(c) * scale
on the kernels of csrc/fp8q_ocp.hip (include/fp8q.h states the arithmetic; the oracle is torch's CPU cast).  The codes with
`scale` as a per-row [C, 1] or per-tensor [1] factor are the operands a scaled FP8 matrix multiplication takes.

It follows the quantizer protocol (QuantizerBase), so QuantizationManager drives it with the min/max estimators and the
model zoo takes it as `method=OCPFP8Quantizer`; it is deliberately NOT a member of QMethods (the CLI's choices).  Forward
only: there is no backward kernel, and a call that would need a gradient raises NotImplementedError.  The MSE and line-search
estimators are not supported with it.  There is no CPU path.

OCPBlockFP8Quantizer, below it, is the same format under a float32 scale per 1x128 / 128x1 / 128x128 tile
(csrc/fp8q_ocp_block.hip): range-free, like MXQuantizer, because a tile's scale is found inside the quantizing pass.

Both take stochastic=True, seed=...: the codes are then rounded stochastically instead of to nearest even (include/fp8q.h: 16
bits of Philox4x32-10 per element), which is what the operands of a backward product want; the seeds are counted as
MXQuantizer counts them (`last_seed`, reseed()).
"""
import torch

from fp8q import ops as _ops
from .fp8 import QuantizerBase, QuantizerNotInitializedError

_HALF = (torch.float16, torch.bfloat16)


class _Stochastic:
    """MXQuantizer's seed bookkeeping for the two quantizers below: with stochastic=True, call number n of forward / encode
    (/ encode_t / encode_both) uses the seed (seed + n) mod 2^64 and records it as `last_seed`, so that the op with
    seed=q.last_seed reproduces the call; reseed(seed) starts the count again."""

    def _init_stochastic(self, stochastic, seed):
        self.stochastic = stochastic
        self.reseed(seed)

    @staticmethod
    def _check_stochastic(stochastic, seed):
        if not isinstance(stochastic, bool):
            raise ValueError(f"stochastic must be True or False, got {stochastic!r}")
        _Stochastic._check_seed(seed)

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

    def _sr_repr(self):
        return f", stochastic=True, seed={self.seed}" if self.stochastic else ""


class OCPFP8Quantizer(_Stochastic, QuantizerBase):
    def __init__(self, n_bits=8, fmt=torch.float8_e4m3fn, per_channel=False, eps=1e-8, keep_dtype=False, scale_domain=None,
                 stochastic=False, seed=0, **kwargs):
        if n_bits != 8:
            raise ValueError(f"hardware FP8 has 8 bits, got n_bits={n_bits}")
        if fmt not in _ops.OCP_FMAX:
            raise ValueError(f"fmt must be torch.float8_e4m3fn or torch.float8_e5m2, got {fmt}")
        self._check_stochastic(stochastic, seed)
        super().__init__(n_bits=n_bits, per_channel=per_channel, **kwargs)
        self.fmt = fmt
        self.eps = eps
        self._init_stochastic(stochastic, seed)
        # float16 / bfloat16 inputs: False returns float32 (the manager widens them), True the input's dtype (rounded once)
        self.keep_dtype = keep_dtype
        # the range, float32 [1] or [C] on the device; named apart from FPQuantizer's `maxval`, whose holders the layers'
        # quantized-weight cache takes for FPQuantizers
        self.register_buffer("_maxval", None)

    def __setattr__(self, name, value):
        if name == "_maxval":       # every assignment of the range starts a new range epoch, as on the other quantizers
            object.__setattr__(self, "_range_epoch", getattr(self, "_range_epoch", 0) + 1)
        super().__setattr__(name, value)

    @property
    def is_initialized(self):
        return self._maxval is not None

    @property
    def symmetric(self):
        return True

    @property
    def fmax(self):
        return _ops.OCP_FMAX[self.fmt]

    @property
    def range_maxval(self):
        if self._maxval is None:
            raise QuantizerNotInitializedError()
        return self._maxval

    @property
    def scale(self):
        """max(maxval, eps) / fmax, float32 [1] or [C]: the kernels' own values (fp8q.ops.ocp_scale)"""
        return _ops.ocp_scale(self.range_maxval, self.fmt, self.eps)

    def reset(self):
        self._maxval = None

    def set_quant_range(self, x_min, x_max):
        """maxval = max(|x_min|, |x_max|), kept on the device: nothing is read back"""
        self.x_min_fp32, self.x_max_fp32 = x_min, x_max
        if not isinstance(x_min, torch.Tensor):
            x_min, x_max = torch.tensor(float(x_min)), torch.tensor(float(x_max))
        if x_min.numel() > 1 and not self.per_channel:
            raise ValueError("x_min and x_max must be a float or 1-element tensor for per-tensor quantization "
                             "(per_channel=False)")
        mv = torch.max(x_min.detach().abs(), x_max.detach().abs()).to(torch.float32).reshape(-1)
        if self._maxval is not None and self._maxval.device != mv.device:
            mv = mv.to(self._maxval.device)
        self._maxval = mv

    def _range_for(self, t):
        mv = self.range_maxval
        if mv.device != t.device:
            mv = self._maxval = mv.to(t.device)
        if mv.numel() != 1 and not (self.per_channel and t.dim() > 0 and t.shape[0] == mv.numel()):
            raise _ops.Fp8qError(f"the range has {mv.numel()} entries, the tensor {tuple(t.shape)}")
        return mv

    def forward(self, x_float):
        if torch.is_grad_enabled() and x_float.requires_grad:
            raise NotImplementedError("OCPFP8Quantizer is forward-only: there is no backward kernel for the hardware FP8 "
                                      "lane (call it under torch.no_grad(), or on a detached tensor)")
        out_dtype = x_float.dtype if (self.keep_dtype and x_float.dtype in _HALF) else None
        return _ops.ocp_quantize(x_float, self._range_for(x_float), self.fmt, self.eps, out_dtype=out_dtype, **self._draw())

    def encode(self, x_float):
        """The codes of forward(x): a torch.float8_e4m3fn / torch.float8_e5m2 tensor shaped like x; `scale` goes with them."""
        return _ops.ocp_encode(x_float.detach(), self._range_for(x_float), self.fmt, self.eps, want_scale=False,
                               **self._draw())[0]

    def decode(self, codes, out_dtype=None):
        """Values of encode()'s codes, float32 or out_dtype (float16 / bfloat16: the float32 value rounded once):
        decode(encode(x)) == forward(x) bit for bit."""
        self._range_for(codes)
        return _ops.ocp_decode(codes, self.scale, out_dtype=out_dtype, fmt=self.fmt)

    def make_range_trainable(self):
        raise NotImplementedError("OCPFP8Quantizer is forward-only: its range cannot be learned")

    def fix_ranges(self):
        pass

    def extra_repr(self):
        name = "E4M3FN" if self.fmt == torch.float8_e4m3fn else "E5M2"
        return f"{super().extra_repr()}, fmt={name}, eps={self.eps}{self._sr_repr()}"


class OCPBlockFP8Quantizer(_Stochastic, QuantizerBase):
    """The same formats under one float32 scale per TILE of (1, 128), (128, 1) or (128, 128) elements -- the operands of a
    block-scaled FP8 matrix multiplication (csrc/fp8q_ocp_block.hip): 1x128 along the reduction dimension for activations,
    128x128 for weights, 128x1 for the operand of a product that reduces over dim 0.  The scale of a tile is a function of
    that tile's own largest element, found inside the quantizing pass: there is no range to estimate, calibrate, fix or learn,
    and `range_free = True` tells QuantizationManager so, as on MXQuantizer.  flatten_rows=True views a tensor of more than
    two dimensions as [shape[0], -1] first (a convolution weight); the tiles that span rows need a matrix after that.
        forward(x) = decode(*encode(x)),   encode(x) = (codes, scales) of fp8q.ops.ocp_block_encode
    Forward only, not a member of QMethods, no CPU path; the model zoo takes it as `method=OCPBlockFP8Quantizer`."""
    range_free = True

    def __init__(self, n_bits=8, fmt=torch.float8_e4m3fn, tile=(1, 128), eps=1e-8, keep_dtype=False, flatten_rows=False,
                 per_channel=False, scale_domain=None, stochastic=False, seed=0, **kwargs):
        if n_bits != 8:
            raise ValueError(f"hardware FP8 has 8 bits, got n_bits={n_bits}")
        if fmt not in _ops.OCP_FMAX:
            raise ValueError(f"fmt must be torch.float8_e4m3fn or torch.float8_e5m2, got {fmt}")
        try:
            tile = _ops._ocpb_tile(tile)
        except _ops.Fp8qError as e:
            raise ValueError(str(e)) from None
        if not (isinstance(eps, (int, float)) and not isinstance(eps, bool) and eps >= 0):
            raise ValueError(f"eps must be a non-negative number, got {eps!r}")
        self._check_stochastic(stochastic, seed)
        # per_channel is the protocol's argument; the scales are per tile either way
        super().__init__(n_bits=n_bits, per_channel=per_channel, **kwargs)
        self.fmt = fmt
        self.tile = tile
        self.eps = eps
        # float16 / bfloat16 inputs: False returns float32, True the input's dtype (the float32 value rounded once)
        self.keep_dtype = keep_dtype
        self.flatten_rows = flatten_rows
        self._init_stochastic(stochastic, seed)

    @property
    def is_initialized(self):
        return True

    @property
    def symmetric(self):
        return True

    @property
    def fmax(self):
        return _ops.OCP_FMAX[self.fmt]

    def reset(self):
        pass

    def set_quant_range(self, x_min, x_max):
        pass

    def fix_ranges(self):
        pass

    def make_range_trainable(self):
        raise NotImplementedError("OCPBlockFP8Quantizer is forward-only and has no range: nothing can be learned")

    def _rows(self, t):
        """t as the kernels cut it into tiles: of [shape[0], -1] with flatten_rows"""
        if self.flatten_rows and t.dim() > 2:
            return t.contiguous().view(t.shape[0], -1)
        return t

    def forward(self, x_float):
        if torch.is_grad_enabled() and x_float.requires_grad:
            raise NotImplementedError("OCPBlockFP8Quantizer is forward-only: there is no backward kernel for the hardware "
                                      "FP8 lane (call it under torch.no_grad(), or on a detached tensor)")
        out_dtype = x_float.dtype if (self.keep_dtype and x_float.dtype in _HALF) else None
        y = _ops.ocp_block_quantize(self._rows(x_float), self.fmt, self.tile, self.eps, out_dtype=out_dtype, **self._draw())
        return y.view(x_float.shape)

    def encode(self, x_float):
        """(codes, scales) of forward(x): codes of dtype `fmt` shaped like x (with flatten_rows: like its [shape[0], -1]
        view), scales float32, one per tile (fp8q.ops.ocp_block_encode)"""
        return _ops.ocp_block_encode(self._rows(x_float.detach()), self.fmt, self.tile, self.eps, **self._draw())

    def decode(self, codes, scales, out_dtype=None):
        """Values of encode()'s operands, float32 or out_dtype (float16 / bfloat16: the float32 value rounded once), shaped as
        encode() saw them: decode(*encode(x)) == forward(x) bit for bit (after .view(x.shape) with flatten_rows)."""
        return _ops.ocp_block_decode(codes, scales, self.tile, out_dtype=out_dtype, fmt=self.fmt)

    def _transposable(self):
        if self.tile not in _ops.OCP_BLOCK_T_TILES:
            raise ValueError(f"a quantizer with tile={self.tile} has no transposed operands: they are made under (1, 128) or "
                             f"(128, 128) tiles (fp8q.ops.ocp_block_encode_t)")

    def encode_t(self, x_float):
        """(codes_t, scales_t): the operands of the transpose of the matrix encode() sees -- encode(x.t().contiguous()) byte
        for byte, from x as it lies (fp8q.ops.ocp_block_encode_t).  x must be a matrix (after flatten_rows);
        decode(codes_t, scales_t) gives the transpose's values.  ValueError for a quantizer built with tile=(128, 1)."""
        self._transposable()
        return _ops.ocp_block_encode_t(self._rows(x_float.detach()), self.fmt, self.tile, self.eps, **self._draw())

    def encode_both(self, x_float):
        """(codes, scales, codes_t, scales_t) = encode(x) + encode_t(x) from one read of x (fp8q.ops.ocp_block_encode_both)"""
        self._transposable()
        return _ops.ocp_block_encode_both(self._rows(x_float.detach()), self.fmt, self.tile, self.eps, **self._draw())

    def extra_repr(self):
        name = "E4M3FN" if self.fmt == torch.float8_e4m3fn else "E5M2"
        return f"{super().extra_repr()}, fmt={name}, tile={self.tile[0]}x{self.tile[1]}, eps={self.eps}, " \
               f"flatten_rows={self.flatten_rows}{self._sr_repr()}"
