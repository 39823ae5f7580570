"""Uniform (INT) fake-quantizers -- the INT baseline of the FP8 study (compute_quant_error.py config 1, --qmethod-act).

Reference: quantization/quantizers/uniform_quantizers.py:13-331.  On CUDA fp32 tensors in the linear scale domain
`forward` and `set_quant_range` run the HIP kernels of csrc/fp8q_int.hip (one launch each, the symmetric sign read from
device memory: no host round trip).  Under autograd -- x or a learned range (`make_range_trainable`) wants a gradient --
`forward` goes through _IntFakeQuantSTE: the same forward kernel, and ONE backward kernel (csrc/fp8q_intgrad.hip) for d/dx,
d/ddelta and d/dzero_float, LSQ's `grad_scaling` included.  Everything else -- CPU, other dtypes, the log domain, a custom
discretizer -- is the reference's torch op chain.  FP8Q_INT_KERNELS=0 forces that chain, FP8Q_GRAD_KERNELS=0 forces it
under autograd only (the switch of the FP quantizer's backward).

The integers themselves (csrc/fp8q_intcodec.hip): `to_integer_forward` runs fp8q.ops.int_to_integer under forward's kernel
conditions and stays the torch chain otherwise; `encode` / `decode` give and take the 1- or 2-byte storage codes and exist on
the kernel path only (they raise elsewhere, FP8Q_INT_KERNELS=0 included).

float16 / bfloat16 tensors (csrc/fp8q_inth16.hip): a quantizer built with `keep_dtype=True` runs `forward` and the
range-setting forwards on the half kernels under the same conditions and returns x's dtype -- x widened exactly, the fp32
chain, one rounding back; the ranges stay float32.  Under autograd or with learned ranges such an x is widened, takes the
float32 route above and the result is cast back.  Without keep_dtype a half tensor is the eager chain, as ever.

The producer epilogue (csrc/fp8q_intepilogue.hip): a per-tensor quantizer built with `fuse_epilogue=True` lets its
QuantizationManager run eval-mode batch norm + residual + ReLU / ReLU6 + this quantizer as ONE kernel (`can_fuse` /
`forward_fused`), bit for bit fp8q.ops.int_quantize of fp8q.ops.affine_act.  Off by default, because the fused batch norm
rounds as ATen's CPU kernel does and the CUDA batch_norm of the unfused chain differs from it in the last bit.

The integer codes of half tensors (csrc/fp8q_codec_h16.hip): with `keep_dtype=True`, `encode` takes a float16 / bfloat16
tensor under forward's kernel conditions (the codes of the exactly widened tensor) and `decode(codes, out_dtype=...)` returns
float16 / bfloat16 values (the float32 value rounded once), so decode(encode(x), out_dtype=x.dtype) == forward(x) bit for bit
wherever x is not NaN.  `to_integer_forward` stays float32-only.
"""
import os

import torch

from fp8q import ops as _ops
from .fp8 import QuantizerBase, QuantizerNotInitializedError, _grad_kernels, round_ste_func


def _int_kernels_enabled():
    return os.environ.get("FP8Q_INT_KERNELS", "1") != "0"


class _ScaleGradient(torch.autograd.Function):
    """identity forward, the gradient times a constant backward (reference rounding_utils.py: scale_grad_func)"""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x

    @staticmethod
    def backward(ctx, grad):
        return grad * ctx.scale, None


scale_grad_func = _ScaleGradient.apply


class _IntFakeQuantSTE(torch.autograd.Function):
    """fp8q.ops.int_quantize forward, fp8q.ops.int_quantize_backward backward: what autograd derives from the op chain
    scale * (clamp(round_ste(x / scale) + zp, int_min, int_max) - zp) (include/fp8q.h states the arithmetic), computed
    only for the inputs that need a gradient.  The forward keeps x and the ranges, not its result."""

    @staticmethod
    def forward(ctx, x, delta, zero_float, signed_flag, n_bits, symmetric, eps, grad_scale_elems):
        y = _ops.int_quantize(x.detach(), delta.detach(), None if zero_float is None else zero_float.detach(), signed_flag,
                              n_bits, symmetric, eps)
        ctx.save_for_backward(x, delta, zero_float, signed_flag)
        ctx.cfg = (n_bits, symmetric, eps, grad_scale_elems)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, delta, zero_float, signed_flag = ctx.saved_tensors
        need_x, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_z = zero_float is not None and ctx.needs_input_grad[2]
        if not (grad.is_cuda and grad.dtype == torch.float32):      # y is CUDA float32, so its gradient is too
            raise _ops.Fp8qError(f"_IntFakeQuantSTE.backward: expected a CUDA float32 gradient, got {grad.dtype} on {grad.device}")
        if not (need_x or need_d or need_z):
            return (None,) * 8
        n_bits, symmetric, eps, gs_elems = ctx.cfg
        gx, gd, gz = _ops.int_quantize_backward(x, grad, delta, zero_float, signed_flag, n_bits, symmetric, eps, need_x,
                                                need_d, need_z, gs_elems)
        if need_d:
            gd = gd.reshape(delta.shape)
        if need_z:
            gz = gz.reshape(zero_float.shape)
        return gx, gd, gz, None, None, None, None, None


class AsymmetricUniformQuantizer(QuantizerBase):
    _RANGE_BUFFERS = ("_delta", "_zero_float", "_signed")

    def __setattr__(self, name, value):
        # every assignment of a range buffer starts a new range epoch (the layers' quantized-weight cache keys on it,
        # as on FPQuantizer's); the kernels' in-place range writes bump it themselves
        if name in AsymmetricUniformQuantizer._RANGE_BUFFERS:
            object.__setattr__(self, "_range_epoch", getattr(self, "_range_epoch", 0) + 1)
        super().__setattr__(name, value)

    def _load_from_state_dict(self, *args, **kwargs):
        object.__setattr__(self, "_range_epoch", getattr(self, "_range_epoch", 0) + 1)   # copies in place
        super()._load_from_state_dict(*args, **kwargs)

    def _bump_range_epoch(self):
        object.__setattr__(self, "_range_epoch", getattr(self, "_range_epoch", 0) + 1)

    def _kernel_common(self, dev):
        """The quantizer side of the kernel path's conditions (see the module docstring)."""
        n = self.n_bits
        return (self.scale_domain == "linear" and self.discretizer is round_ste_func and dev.type == "cuda"
                and isinstance(n, int) and 2 <= n <= 16 and _int_kernels_enabled())

    def _kernel_buffers_ok(self, dev):
        """Fixed ranges on the kernel path: plain fp32 buffers (not range Parameters) on `dev`."""
        d = self._delta
        if not (isinstance(d, torch.Tensor) and not isinstance(d, torch.nn.Parameter) and d.dtype == torch.float32
                and d.device == dev and not d.requires_grad):
            return False
        if self.symmetric:
            sg = self._signed
            return isinstance(sg, torch.Tensor) and sg.dtype == torch.bool and sg.device == dev and sg.numel() == 1
        z = self._zero_float
        return (isinstance(z, torch.Tensor) and not isinstance(z, torch.nn.Parameter) and z.dtype == torch.float32
                and z.device == dev and z.numel() == d.numel() and not z.requires_grad)

    def _half_kept(self, x):
        """x is a CUDA float16 / bfloat16 tensor and this quantizer keeps its dtype"""
        return (getattr(self, "keep_dtype", False) and isinstance(x, torch.Tensor) and x.is_cuda
                and x.dtype in (torch.float16, torch.bfloat16))

    def _kernel_x_ok(self, x, n, half_ok=False):
        """x takes the forward kernels for a range of n entries; half_ok: a kept half tensor does too (the half lane)"""
        if not (isinstance(x, torch.Tensor) and (x.dtype == torch.float32 or (half_ok and self._half_kept(x))) and x.is_cuda
                and not (x.requires_grad and torch.is_grad_enabled())):
            return False
        return n == 1 or (self.per_channel and x.dim() > 0 and x.shape[0] == n)

    def _grad_kernel_ok(self, x, dev):
        """The autograd route: x CUDA fp32, fp32 ranges on x's device (Parameters or buffers), something wants a gradient."""
        if not (torch.is_grad_enabled() and _grad_kernels() and isinstance(x, torch.Tensor) and x.is_cuda
                and x.dtype == torch.float32):
            return False
        d, z = self._delta, (None if self.symmetric else self._zero_float)

        def fp32_here(t):
            return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == dev

        if not fp32_here(d) or not (d.numel() == 1 or (self.per_channel and x.dim() > 0 and x.shape[0] == d.numel())):
            return False
        if self.symmetric:
            sg = self._signed
            if not (isinstance(sg, torch.Tensor) and sg.dtype == torch.bool and sg.device == dev and sg.numel() == 1):
                return False
        elif not (fp32_here(z) and z.numel() == d.numel()):
            return False
        return x.numel() > 0 and (x.requires_grad or d.requires_grad or (z is not None and z.requires_grad))

    def _grad_scale_elems(self, x):
        """calculate_grad_scale's element count (0: no gradient scaling)"""
        if not self.grad_scaling:
            return 0
        return x.numel() // x.shape[0] if self.per_channel else x.numel()

    def _range_out(self, x_min):
        """The range buffers the kernels write: the current ones in place when they fit, fresh ones otherwise."""
        def fits(t, shape, dtype):
            return (isinstance(t, torch.Tensor) and not isinstance(t, torch.nn.Parameter) and t.shape == shape
                    and t.dtype == dtype and t.device == x_min.device and t.is_contiguous())
        d = self._delta if fits(self._delta, x_min.shape, torch.float32) else None
        if self.symmetric:
            return d, None, self._signed if fits(self._signed, torch.Size(()), torch.bool) else None
        return d, self._zero_float if fits(self._zero_float, x_min.shape, torch.float32) else None, None

    def _range_kernel_ok(self, x_min, x_max):
        if not (isinstance(x_min, torch.Tensor) and isinstance(x_max, torch.Tensor)):
            return False
        if not self._kernel_common(x_min.device):
            return False
        if (x_min.dtype != torch.float32 or x_max.dtype != torch.float32 or x_max.device != x_min.device
                or x_min.shape != x_max.shape or x_min.numel() == 0):
            return False
        if torch.is_grad_enabled() and (x_min.requires_grad or x_max.requires_grad):
            return False
        if isinstance(self._delta, torch.nn.Parameter) or isinstance(self._zero_float, torch.nn.Parameter):
            return False
        return self.per_channel or x_min.numel() == 1      # per tensor with a vector: the eager path raises

    def _store_range(self, delta, zero_float, signed_flag):
        self._delta = delta
        if self.symmetric:
            self._signed = signed_flag
        else:
            self._zero_float = zero_float
        self._bump_range_epoch()

    def _range_forward(self, x, x_min, x_max):
        """set_quant_range(x_min, x_max) then forward(x); ONE launch on the kernel path."""
        if (self._range_kernel_ok(x_min, x_max) and self._kernel_x_ok(x, x_min.numel(), half_ok=True)
                and x.device == x_min.device):
            self.x_min_fp32, self.x_max_fp32 = x_min, x_max
            y, d, z, sg = _ops.int_range_quantize(x, x_min, x_max, self.n_bits, self.symmetric, self.eps,
                                                  *self._range_out(x_min), out_dtype=x.dtype)
            self._store_range(d, z, sg)
            return y
        self.set_quant_range(x_min, x_max)
        return self(x)

    def _minmax_forward(self, x):
        """Per-channel current_minmax + set_quant_range + forward (weights), or None off the kernel path.
        Returns (y, row_min, row_max)."""
        if not (self.per_channel and x.dim() > 0 and x.numel() > 0 and self._kernel_common(x.device)
                and self._kernel_x_ok(x, x.shape[0], half_ok=True) and not isinstance(self._delta, torch.nn.Parameter)
                and not isinstance(self._zero_float, torch.nn.Parameter)):
            return None
        like = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        y, mn, mx, d, z, sg = _ops.int_minmax_quantize(x, self.n_bits, self.symmetric, self.eps,
                                                       *self._range_out(like), out_dtype=x.dtype)
        self.x_min_fp32, self.x_max_fp32 = mn, mx
        self._store_range(d, z, sg)
        return y, mn, mx

    def __init__(self, n_bits, scale_domain="linear", discretizer=round_ste_func, discretizer_args=tuple(),
                 grad_scaling=False, eps=1e-8, keep_dtype=False, fuse_epilogue=False, **kwargs):
        super().__init__(n_bits=n_bits, **kwargs)
        # True lets QuantizationManager.can_fuse hand the producer's batch norm / residual / activation to the fused INT
        # epilogue (csrc/fp8q_intepilogue.hip).  Off by default: the fused batch norm is ATen's CPU arithmetic (the fma form),
        # which differs in the last bit from the CUDA batch_norm kernel of the unfused chain.  A setting, not state.
        self.fuse_epilogue = fuse_epilogue
        # float16 / bfloat16 inputs: True runs the half kernels and returns x's dtype (widen exactly, the fp32 chain, one
        # rounding back); False leaves such a tensor to the eager chain (the manager widens it and returns float32)
        self.keep_dtype = keep_dtype
        assert scale_domain in ("linear", "log")
        self.register_buffer("_delta", None)
        self.register_buffer("_zero_float", None)
        self.discretizer = discretizer(*discretizer_args) if isinstance(discretizer, type) else discretizer
        self.scale_domain = scale_domain
        self.grad_scaling = grad_scaling
        self.eps = eps

    @property
    def delta(self):
        if self._delta is None:
            raise QuantizerNotInitializedError()
        return self._delta

    @property
    def zero_float(self):
        if self._zero_float is None:
            raise QuantizerNotInitializedError()
        return self._zero_float

    @property
    def is_initialized(self):
        return self._delta is not None

    @property
    def symmetric(self):
        return False

    @property
    def int_min(self):
        return 0.0

    @property
    def int_max(self):
        return 2.0 ** self.n_bits - 1

    @property
    def scale(self):
        return torch.clamp(self.delta, min=self.eps) if self.scale_domain == "linear" else torch.exp(self.delta)

    @property
    def zero_point(self):
        return torch.clamp(self.discretizer(self.zero_float), self.int_min, self.int_max)

    @property
    def x_max(self):
        return self.scale * (self.int_max - self.zero_point)

    @property
    def x_min(self):
        return self.scale * (self.int_min - self.zero_point)

    def _params_like(self, x):
        scale, zp = self.scale, self.zero_point
        if torch.is_tensor(scale) and scale.device != x.device:
            scale = scale.to(x.device)
        if torch.is_tensor(zp) and zp.device != x.device:
            zp = zp.to(x.device)
        if self.per_channel and torch.is_tensor(scale) and scale.dim() == 1 and x.dim() > 1:
            shape = [-1] + [1] * (x.dim() - 1)
            scale = scale.view(shape)
            zp = zp.view(shape) if torch.is_tensor(zp) and zp.dim() == 1 else zp
        return scale, zp

    def calculate_grad_scale(self, quant_tensor):
        """LSQ's 1 / sqrt(Qp * N): N the elements of a channel (per channel) or of the tensor"""
        n = quant_tensor.numel()
        if self.per_channel:
            n /= quant_tensor.shape[0]
        return (self.int_max * n) ** -0.5

    def _chain_params(self, x):
        """_params_like, with the gradients of scale and zero point scaled when grad_scaling is set"""
        scale, zp = self._params_like(x)
        if self.grad_scaling and torch.is_grad_enabled():
            gs = self.calculate_grad_scale(x)
            scale = scale_grad_func(scale, gs)
            if not self.symmetric:
                zp = scale_grad_func(zp, gs)
        return scale, zp

    def _fixed_kernel_ok(self, t, x_like=True):
        """forward's conditions for ops.int_quantize: kernels on, fixed fp32 range buffers on t's device, and (x_like) t a
        CUDA fp32 tensor nothing wants a gradient of, shaped for the range."""
        d = self._delta
        return (d is not None and isinstance(t, torch.Tensor) and self._kernel_common(t.device)
                and self._kernel_buffers_ok(t.device) and (not x_like or self._kernel_x_ok(t, d.numel())))

    def _range_args(self):
        return (self._delta, None if self.symmetric else self._zero_float, self._signed if self.symmetric else None,
                self.n_bits, self.symmetric, self.eps)

    def to_integer_forward(self, x_float, *args, **kwargs):
        if self._fixed_kernel_ok(x_float):
            return _ops.int_to_integer(x_float, *self._range_args())
        scale, zp = self._chain_params(x_float)
        return torch.clamp(self.discretizer(x_float / scale) + zp, self.int_min, self.int_max)

    def encode(self, x_float):
        """The integers of forward(x) as storage codes (fp8q.ops.int_encode: uint8 up to 8 bits, int16 beyond, raw
        two's-complement bits).  Kernel path only -- the conditions of forward's, a float16 / bfloat16 tensor with keep_dtype
        included; anything else raises."""
        d = self._delta
        if not (self._fixed_kernel_ok(x_float, x_like=False) and self._kernel_x_ok(x_float, d.numel(), half_ok=True)):
            raise _ops.Fp8qError("encode needs the INT kernels: a CUDA float32 tensor (float16 / bfloat16 with keep_dtype) "
                                 "without a gradient, fixed float32 range buffers on its device, the linear scale domain, and "
                                 "FP8Q_INT_KERNELS not 0")
        return _ops.int_encode(x_float, *self._range_args())

    def decode(self, codes, out_dtype=None):
        """Values of encode()'s codes, float32 or out_dtype (float16 / bfloat16: the float32 value rounded once):
        decode(encode(x)) == forward(x) bit for bit wherever x is not NaN."""
        d = self._delta
        if not (self._fixed_kernel_ok(codes, x_like=False) and codes.is_cuda and not codes.is_floating_point()
                and (d.numel() == 1 or (self.per_channel and codes.dim() > 0 and codes.shape[0] == d.numel()))):
            raise _ops.Fp8qError("decode needs the INT kernels: CUDA integer codes, fixed float32 range buffers on their "
                                 "device, the linear scale domain, and FP8Q_INT_KERNELS not 0")
        return _ops.int_decode(codes, *self._range_args(), out_dtype=out_dtype)

    def forward(self, x_float, *args, **kwargs):
        d = self._delta
        if (d is not None and self._kernel_common(x_float.device) and self._kernel_buffers_ok(x_float.device)
                and self._kernel_x_ok(x_float, d.numel(), half_ok=True)):
            return _ops.int_quantize(x_float, d, None if self.symmetric else self._zero_float,
                                     self._signed if self.symmetric else None, self.n_bits, self.symmetric, self.eps,
                                     out_dtype=x_float.dtype)
        if self._half_kept(x_float) and self._kernel_common(x_float.device):
            # under autograd, or with learned ranges: widen, the float32 route (its kernels where they apply), cast back
            return self.forward(x_float.float()).to(x_float.dtype)
        if d is not None and self._kernel_common(x_float.device) and self._grad_kernel_ok(x_float, x_float.device):
            return _IntFakeQuantSTE.apply(x_float, d, None if self.symmetric else self._zero_float,
                                          self._signed if self.symmetric else None, self.n_bits, self.symmetric, self.eps,
                                          self._grad_scale_elems(x_float))
        scale, zp = self._chain_params(x_float)
        return scale * (self.to_integer_forward(x_float) - zp)

    def _tensorize_min_max(self, x_min, x_max):
        if not torch.is_tensor(x_min):
            x_min, x_max = torch.tensor(x_min).float(), torch.tensor(x_max).float()
        if x_min.dim() > 0 and len(x_min) > 1 and not self.per_channel:
            raise ValueError("x_min and x_max must be a float or 1-D Tensor for per-tensor quantization "
                             "(per_channel=False)")
        # the range always contains zero; a positive upper end avoids a zero scale
        return torch.min(x_min, torch.zeros_like(x_min)), torch.max(x_max, torch.ones_like(x_max) * self.eps)

    def set_quant_range(self, x_min, x_max):
        self.x_min_fp32, self.x_max_fp32 = x_min, x_max
        if self._range_kernel_ok(x_min, x_max):
            d, z, sg = _ops.int_set_range(x_min, x_max, self.n_bits, self.symmetric, self.eps, *self._range_out(x_min))
            self._store_range(d, z, sg)
            return
        x_min, x_max = self._tensorize_min_max(x_min, x_max)
        delta = (x_max - x_min) / self.int_max
        self._zero_float = (-x_min / delta).detach()
        self._delta = (torch.log(delta) if self.scale_domain == "log" else delta).detach()

    def make_range_trainable(self):
        if not isinstance(self._delta, torch.nn.Parameter):
            self._delta = torch.nn.Parameter(self._delta)
            if self._zero_float is not None:
                self._zero_float = torch.nn.Parameter(self._zero_float)

    def fix_ranges(self):
        for name in ("_delta", "_zero_float"):
            p = getattr(self, name, None)
            if isinstance(p, torch.nn.Parameter):
                delattr(self, name)
                self.register_buffer(name, p.data)

    def generate_grid(self):
        return self.scale * (torch.arange(self.int_min, self.int_max + 1, device=self.delta.device) - self.zero_point)


class SymmetricUniformQuantizer(AsymmetricUniformQuantizer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("_signed", None)

    @property
    def signed(self):
        if self._signed is None:
            raise QuantizerNotInitializedError()
        return self._signed.item()

    @property
    def symmetric(self):
        return True

    @property
    def int_min(self):
        return -(2.0 ** (self.n_bits - 1)) if self.signed else 0

    @property
    def int_max(self):
        return 2.0 ** (self.n_bits - self.signed) - 1

    @property
    def zero_point(self):
        return 0.0

    def set_quant_range(self, x_min, x_max):
        self.x_min_fp32, self.x_max_fp32 = x_min, x_max
        if self._range_kernel_ok(x_min, x_max):
            d, _, sg = _ops.int_set_range(x_min, x_max, self.n_bits, True, self.eps, *self._range_out(x_min))
            self._store_range(d, None, sg)
            return
        x_min, x_max = self._tensorize_min_max(x_min, x_max)
        self._signed = x_min.min() < 0
        delta = torch.max(x_min.abs(), x_max) / self.int_max
        self._delta = (torch.log(delta) if self.scale_domain == "log" else delta).detach()
