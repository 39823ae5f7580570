"""Torch-facing wrappers of the C ABI: tensors in, tensors out, launched on the current stream.

PyTorch is used for device memory and streams only; all arithmetic is in libfp8q_hip.so.
"""
import torch

from ._lib import Fp8qError, check, lib

FOLD_CURRENT, FOLD_ALL, FOLD_RUNNING = 0, 1, 2

_ws_cache = {}
_ws_retired = []     # outgrown min/max workspaces, not yet inspected by check_workspaces()
_mm_ws_bytes = {}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    """raw hipStream_t of torch's current stream on t's device (fast path avoids a Stream object)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _on_device:
    """`with _on_device(t):` -- make t's device current for the launch; a no-op (and no torch call
    beyond one integer query) when it already is, which is the single-GPU-per-process case."""
    __slots__ = ("idx", "prev")

    def __init__(self, t):
        self.idx = t.device.index
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def _require(t, name, dtype=torch.float32, like=None):
    """t is a CUDA(HIP) tensor of `dtype` (a dtype or a tuple of them), on `like`'s device when given."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise Fp8qError(f"{name} must be a CUDA(HIP) tensor: the FP8 engine has no CPU path")
    if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        want = " or ".join(str(d).replace("torch.", "") for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
        raise Fp8qError(f"{name} must be {want}, got {t.dtype}")
    if like is not None and t.device != like.device:
        raise Fp8qError(f"{name} is on {t.device}, expected {like.device} (all tensors of a call live on one device)")


def _out(out, like, dtype=None, name="out"):
    """The output tensor of a launch: a fresh one, or the caller's `out=` after checking that the kernel may write
    like.numel() elements of `dtype` through its raw pointer (same device, dtype, element count, contiguous)."""
    dtype = like.dtype if dtype is None else dtype
    if out is None:
        return torch.empty(like.shape, dtype=dtype, device=like.device)
    _require(out, name, dtype, like)
    if out.numel() != like.numel() or not out.is_contiguous():
        raise Fp8qError(f"{name} must be a contiguous tensor of {like.numel()} elements "
                        f"(got {tuple(out.shape)}, contiguous={out.is_contiguous()})")
    return out


def _dense_flat(x):
    """x as a flat [numel] view over its own storage when x is dense but not contiguous (channels-last activations, a
    transposed matrix: every element of the storage span belongs to x exactly once), else None.  Per-tensor K1 and the
    per-tensor min/max are elementwise / order-free, so they can run on the storage as it lies -- no NCHW copy (8 B per
    element) -- and the result keeps x's strides, as the reference's elementwise ATen ops do."""
    if x.is_contiguous() or x.numel() == 0:
        return None
    dims = sorted((st, sz) for st, sz in zip(x.stride(), x.shape) if sz > 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return None
        expect *= sz
    return x.as_strided((x.numel(),), (1,), x.storage_offset())


def _rows(x, per_channel):
    """[C, inner] view geometry: channel = dim 0 (reference: x.view(x.shape[0], -1))."""
    if per_channel:
        C = x.shape[0] if x.dim() > 0 else 1
        return C, (x.numel() // C if C else 0)
    return 1, x.numel()


def _workspace(dev, nbytes, zeroed=False, kind=None, stream=None):
    """Per-(device, stream) scratch buffer.  zeroed=True: the min/max entry points' workspace, whose leading ticket
    counters must be zero on first use and are left zero by every call (include/fp8q.h) -- allocated zero-filled and
    never shared with the kernels that scribble over their scratch (MSE partial sums).  kind="select": the winner
    selection's buffer -- allocated zero-filled too (its header holds a ticket that every call leaves zero), but the rest
    of it is ordinary scratch, so it is neither shared with the min/max workspace nor inspected by check_workspaces().
    kind="grad": the partial sums of quantize_backward -- zero-filled, left zero by every call, a buffer of its own."""
    if stream is None:       # (callers that make several requests per launch pass the raw stream they already looked up)
        stream = _raw_stream(dev.index) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
    key = (dev.index, stream, zeroed, kind)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None and zeroed:
            # a min/max workspace outgrown: its header may hold a time-out count that nobody has looked at yet -- keep it until
            # the next check_workspaces() instead of dropping the report with the buffer.  Never inspected HERE: that would
            # synchronise inside an unrelated enqueue-only op (and raise another call's failure from it).  The list stays
            # short: a workspace only ever grows, and these buffers are tens of kilobytes.
            _ws_retired.append((key, ws))
        alloc = torch.zeros if (zeroed or kind in ("select", "grad")) else torch.empty
        ws = alloc(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=dev)
        _ws_cache[key] = ws
    return ws


_HALF = (torch.float16, torch.bfloat16)
_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # FP8Q_DT_* (include/fp8q.h)


def _half_out_dtype(x, out, out_dtype):
    """result dtype of a half-lane call: out.dtype when `out` is given, else out_dtype, else float32 (the reference's
    type promotion); only float32 and x.dtype exist"""
    dt = out.dtype if isinstance(out, torch.Tensor) else (torch.float32 if out_dtype is None else out_dtype)
    if dt != torch.float32 and dt != x.dtype:
        raise Fp8qError(f"the output of a {x.dtype} input is float32 or {x.dtype}, not {dt}")
    if out is not None and out_dtype is not None and out_dtype != dt:
        raise Fp8qError(f"out is {dt} but out_dtype is {out_dtype}")
    return dt


def _check_out_dtype(x, out_dtype):
    if out_dtype is not None and out_dtype != x.dtype:
        raise Fp8qError(f"out_dtype: a {x.dtype} input gives a {x.dtype} result (float16 / bfloat16 inputs: float32 or their own)")


_VALUES = (torch.float32,) + _HALF     # what the storage codes are made from and decoded to


def _decode_out_dtype(out, out_dtype):
    """result dtype of a decode: out.dtype when `out` is given, else out_dtype, else float32; codes carry no dtype of their
    own, so float32 and both half types exist.  Argument errors come before the device check, as in _half_out_dtype."""
    dt = out.dtype if isinstance(out, torch.Tensor) else (torch.float32 if out_dtype is None else out_dtype)
    if dt not in _VALUES:
        raise Fp8qError(f"decoded values are float32 or float16 / bfloat16, not {dt}")
    if out is not None and out_dtype is not None and out_dtype != dt:
        raise Fp8qError(f"out is {dt} but out_dtype is {out_dtype}")
    return dt


def _quantize_out_dtype(x, out, out_dtype):
    """result dtype of a quantize-style call on the code lanes: float32 for a float32 x (out_dtype, when given, must say so),
    _half_out_dtype's for a float16 / bfloat16 x"""
    if x.dtype in _HALF:
        return _half_out_dtype(x, out, out_dtype)
    _check_out_dtype(x, out_dtype)
    return torch.float32


def _lane(*dtypes, f32="_f32"):
    """(suffix of the entry point, the FP8Q_DT_* it takes) for a call whose value side(s) have `dtypes`: the _h16 entry with
    its type arguments when the first is float16 / bfloat16, else the float32 entry, which takes none"""
    return ("_h16", tuple(_DT[d] for d in dtypes)) if dtypes[0] in _HALF else (f32, ())


def _run(fn, t, *args):
    """lib().<fn>(*args, stream) on t's device and torch's current stream there; a non-zero status raises"""
    with _on_device(t):
        rc = getattr(lib(), fn)(*args, _stream(t))
    check(rc, fn)


def _codes_fmt(codes, fmt, formats, names, hint):
    """the format of `codes` for a decode: their own dtype when it is one of `formats`, else uint8 codes with fmt= naming it"""
    if not isinstance(codes, torch.Tensor) or not codes.is_cuda:
        raise Fp8qError("codes must be a CUDA(HIP) tensor: the FP8 engine has no CPU path")
    if codes.dtype in formats:
        if fmt is not None and fmt != codes.dtype:
            raise Fp8qError(f"codes are {codes.dtype} but fmt is {fmt}")
        return codes.dtype
    if codes.dtype != torch.uint8:
        raise Fp8qError(f"codes must be {names} or uint8, got {codes.dtype}")
    if fmt is None:
        raise Fp8qError(f"uint8 codes carry no format: pass fmt={hint}")
    return fmt


def _quantize_h16(x, maxval, mbits, n_bits, sign_bits, out, out_dtype):
    """K1 on float16 / bfloat16 (fp8q_quantize_h16): x widened exactly, the fp32 contract, the result stored as float32
    or rounded once to x.dtype"""
    if isinstance(mbits, torch.Tensor) or isinstance(sign_bits, torch.Tensor):
        raise Fp8qError("a device-resident mantissa width / sign flag is float32-only: the half-precision lane takes "
                        f"mbits and sign_bits as numbers (x is {x.dtype}; widen it with .float() for that route)")
    dt = _half_out_dtype(x, out, out_dtype)      # (argument errors before the device check: they need no GPU to be told)
    _require(x, "x", _HALF)
    _require(maxval, "maxval", like=x)
    maxval = maxval.contiguous().view(-1)
    n_mv = maxval.numel()
    flat = _dense_flat(x) if (n_mv == 1 and out is None) else None
    if flat is not None:            # per tensor on a dense non-contiguous layout: the storage as it lies, x's strides kept
        res = torch.empty_like(x, dtype=dt)
        flat_out = _dense_flat(res) if res.stride() == x.stride() else None
        if flat_out is not None:
            _quantize_h16(flat, maxval, mbits, n_bits, sign_bits, flat_out, None)
            return res
    x = x.contiguous()
    C, inner = _rows(x, n_mv != 1)
    if n_mv != 1 and n_mv != C:
        raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
    y = _out(out, x, dtype=dt)
    if x.numel() == 0:
        return y
    with _on_device(x):
        rc = lib().fp8q_quantize_h16(x.data_ptr(), y.data_ptr(), _DT[x.dtype], _DT[dt], C, inner, maxval.data_ptr(), n_mv,
                                     float(mbits), int(n_bits), int(sign_bits), _stream(x))
    check(rc, "fp8q_quantize_h16")
    return y


def quantize(x, maxval, mbits, n_bits=8, sign_bits=1, out=None, out_dtype=None):
    """K1: FP8 quantize+dequantize (fp8_quantizer.py:91-133).  maxval: CUDA fp32 tensor [1] or [C]; x float32 or
    float64; mbits: a number, or a 1-element CUDA float32 tensor (read by the kernel: no host round trip).
    x float16 / bfloat16: the result is float32 (what the reference's type promotion returns) unless `out` or
    out_dtype=x.dtype asks for x's own dtype; mbits and sign_bits are numbers there."""
    if isinstance(x, torch.Tensor) and x.dtype in _HALF:
        return _quantize_h16(x, maxval, mbits, n_bits, sign_bits, out, out_dtype)
    _require(x, "x", (torch.float32, torch.float64))
    _check_out_dtype(x, out_dtype)
    _require(maxval, "maxval", like=x)
    maxval = maxval.contiguous().view(-1)
    n_mv = maxval.numel()
    flat = _dense_flat(x) if (n_mv == 1 and out is None) else None
    if flat is not None:            # per tensor on a dense non-contiguous layout: the storage as it lies, x's strides kept
        res = torch.empty_like(x)                            # (preserve_format: x's strides)
        flat_out = _dense_flat(res) if res.stride() == x.stride() else None
        if flat_out is not None:
            quantize(flat, maxval, mbits, n_bits, sign_bits, out=flat_out)
            return res
    x = x.contiguous()
    C, inner = _rows(x, n_mv != 1)
    if n_mv != 1 and n_mv != C:
        raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
    y = _out(out, x)
    if isinstance(mbits, torch.Tensor) and mbits.is_cuda:
        # mantissa width in DEVICE memory (the MSE estimator's vote, not yet brought to the host): fp8q_quantize_dm_f32
        _require(mbits, "mbits", like=x)
        if mbits.numel() != 1 or x.dtype != torch.float32:
            raise Fp8qError("a device-resident mantissa width must be a 1-element float32 tensor, x float32")
        if isinstance(sign_bits, torch.Tensor):     # ... and the sign still a device flag (sign_fold): fp8q_quantize_dms_f32
            _require(sign_bits, "sign_bits", torch.uint8, like=x)
            if sign_bits.numel() != 1:
                raise Fp8qError("a device-resident sign flag must be a 1-element uint8 tensor")
            with _on_device(x):
                rc = lib().fp8q_quantize_dms_f32(x.data_ptr(), y.data_ptr(), C, inner, maxval.data_ptr(), n_mv,
                                                 mbits.data_ptr(), int(n_bits), sign_bits.data_ptr(), _stream(x))
            check(rc, "fp8q_quantize_dms_f32")
            return y
        with _on_device(x):
            rc = lib().fp8q_quantize_dm_f32(x.data_ptr(), y.data_ptr(), C, inner, maxval.data_ptr(), n_mv,
                                            mbits.data_ptr(), int(n_bits), int(sign_bits), _stream(x))
        check(rc, "fp8q_quantize_dm_f32")
        return y
    if isinstance(sign_bits, torch.Tensor):
        # sign_bits still a flag in DEVICE memory (sign_fold: allow_unsigned decided without a host round trip): fp8q_quantize_ds_f32
        _require(sign_bits, "sign_bits", torch.uint8, like=x)
        if sign_bits.numel() != 1 or x.dtype != torch.float32:
            raise Fp8qError("a device-resident sign flag must be a 1-element uint8 tensor, x float32")
        with _on_device(x):
            rc = lib().fp8q_quantize_ds_f32(x.data_ptr(), y.data_ptr(), C, inner, maxval.data_ptr(), n_mv, float(mbits),
                                            int(n_bits), sign_bits.data_ptr(), _stream(x))
        check(rc, "fp8q_quantize_ds_f32")
        return y
    # float64 input (BASELINE config 1): the reference's chain under ATen's type promotion -- bias in float32,
    # everything downstream of x in float64 (fp8q_quantize_f64)
    fn = lib().fp8q_quantize_f64 if x.dtype == torch.float64 else lib().fp8q_quantize_f32
    with _on_device(x):
        rc = fn(x.data_ptr(), y.data_ptr(), C, inner, maxval.data_ptr(), n_mv, float(mbits), int(n_bits),
                int(sign_bits), _stream(x))
    check(rc, "fp8q_quantize_f64" if x.dtype == torch.float64 else "fp8q_quantize_f32")
    return y


_bwd_ws_bytes = {}


def quantize_backward(x, g, maxval, mbits, n_bits=8, sign_bits=1, need_gx=True, need_gmaxval=True, need_gmbits=False,
                      out=None):
    """Backward of K1 (fp8q_quantize_bwd_f32): d/dx, d/dmaxval and d/dmbits of quantize(x; maxval, mbits) for the upstream
    gradient g, in one pass over x and g -- the forward's result is recomputed in the kernel, nothing but x and maxval has to
    be kept.  x, g: CUDA float32 of the same shape, contiguous (per tensor: any dense layout they share, as quantize());
    maxval: CUDA float32 [1] or [C]; mbits: a number, or a 1-element CUDA float32 tensor (read by the kernel, which then also
    evaluates the clamp test and the factor of d/dmbits: no host round trip).
    out (with need_gx): a contiguous CUDA float32 tensor of x's shape that receives gx, as quantize()'s out; gx is then
    written in x's logical order whatever x's layout.
    Returns (gx | None, gmaxval | None, gmbits | None): gx like x (or out), gmaxval float32 [n_maxval], gmbits float32 [1]."""
    _require(x, "x")
    _require(g, "g", like=x)
    _require(maxval, "maxval", like=x)
    if out is not None:
        _require(out, "out", like=x)
        if not need_gx or out.shape != x.shape or not out.is_contiguous():
            raise Fp8qError("out must be a contiguous tensor of x's shape, and only with need_gx")
    if g.shape != x.shape:
        raise Fp8qError(f"g has shape {tuple(g.shape)}, x {tuple(x.shape)}")
    if not (need_gx or need_gmaxval or need_gmbits):
        raise Fp8qError("quantize_backward: nothing requested")
    maxval = maxval.detach().contiguous().view(-1)
    n_mv = maxval.numel()
    x, g = x.detach(), g.detach()
    flat = _dense_flat(x) if (n_mv == 1 and out is None and g.stride() == x.stride()) else None
    if flat is not None:
        # per tensor on a dense non-contiguous layout shared by x and g: the storage as it lies, gx keeps the strides
        res = torch.empty_like(x) if need_gx else None
        flat_out = _dense_flat(res) if (need_gx and res.stride() == x.stride()) else None
        if not need_gx or flat_out is not None:
            _, gmv, gmb = quantize_backward(flat, _dense_flat(g), maxval, mbits, n_bits, sign_bits, need_gx, need_gmaxval,
                                            need_gmbits, out=flat_out)
            return res, gmv, gmb
    x, g = x.contiguous(), g.contiguous()
    C, inner = _rows(x, n_mv != 1)
    if n_mv != 1 and n_mv != C:
        raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
    if x.numel() == 0:
        raise Fp8qError("quantize_backward of an empty tensor")
    mb_dev = None
    if isinstance(mbits, torch.Tensor) and mbits.is_cuda:
        _require(mbits, "mbits", like=x)
        if mbits.numel() != 1:
            raise Fp8qError("a device-resident mantissa width must be a 1-element float32 tensor")
        mb_dev = mbits.detach()
    gx = (out if out is not None else torch.empty_like(x)) if need_gx else None
    gmv = torch.empty(n_mv, dtype=torch.float32, device=x.device) if need_gmaxval else None
    gmb = torch.empty(1, dtype=torch.float32, device=x.device) if need_gmbits else None
    L = lib()
    ws_ptr, ws_len = None, 0
    stream = _stream(x)
    if need_gmaxval or need_gmbits:
        nbytes = _bwd_ws_bytes.get((C, inner, n_mv))
        if nbytes is None:
            nbytes = _bwd_ws_bytes[(C, inner, n_mv)] = L.fp8q_quantize_bwd_workspace_bytes(C, inner, n_mv)
        ws = _workspace(x.device, nbytes, kind="grad", stream=stream)
        ws_ptr, ws_len = ws.data_ptr(), ws.numel()
    with _on_device(x):
        rc = L.fp8q_quantize_bwd_f32(x.data_ptr(), g.data_ptr(), gx.data_ptr() if need_gx else None, C, inner,
                                     maxval.data_ptr(), n_mv, 0.0 if mb_dev is not None else float(mbits),
                                     mb_dev.data_ptr() if mb_dev is not None else None, int(n_bits), int(sign_bits),
                                     gmv.data_ptr() if need_gmaxval else None, gmb.data_ptr() if need_gmbits else None,
                                     ws_ptr, ws_len, stream)
    check(rc, "fp8q_quantize_bwd_f32")
    return gx, gmv, gmb


def sign_fold(x_min, signed_flag=None):
    """FPQuantizer.set_quant_range's sign decision on the device (fp8_quantizer.py:216-225): the 1-element uint8 flag
    (1 = signed; a fresh one when None) is cleared when every value of x_min is >= 0, and never set again.  Enqueue-only."""
    _require(x_min, "x_min")
    if signed_flag is None:
        signed_flag = torch.ones(1, dtype=torch.uint8, device=x_min.device)
    _require(signed_flag, "signed_flag", torch.uint8, like=x_min)
    xm = x_min.detach().contiguous().view(-1)
    with _on_device(xm):
        rc = lib().fp8q_sign_fold_u8(xm.data_ptr(), xm.numel(), signed_flag.data_ptr(), _stream(xm))
    check(rc, "fp8q_sign_fold_u8")
    return signed_flag


def _pack_descs(items):
    """ctypes descriptor array of (x, maxval, mbits[, n_bits[, sign_bits[, out]]]) items; returns (descs, outs, keep)."""
    from ._lib import TensorDesc
    descs = (TensorDesc * len(items))()
    outs, keep = [], []
    dev0 = None
    for d, it in zip(descs, items):
        x, maxval, mbits = it[0], it[1], it[2]
        n_bits = it[3] if len(it) > 3 else 8
        sign_bits = it[4] if len(it) > 4 else 1
        out = it[5] if len(it) > 5 else None
        _require(x, "x")
        _require(maxval, "maxval", like=x)
        if dev0 is None:
            dev0 = x.device
        elif x.device != dev0:
            raise Fp8qError("multi_quantize: all tensors must be on one device")
        x = x.contiguous()
        maxval = maxval.contiguous().view(-1)
        n_mv = maxval.numel()
        C, inner = _rows(x, n_mv != 1)
        if n_mv != 1 and n_mv != C:
            raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
        y = _out(out, x)
        d.x, d.y, d.maxval = x.data_ptr(), y.data_ptr(), maxval.data_ptr()
        d.C, d.inner, d.n_maxval = C, inner, n_mv
        d.mbits, d.n_bits, d.sign_bits = float(mbits), int(n_bits), int(sign_bits)
        outs.append(y)
        keep.append((x, maxval))
    return descs, outs, keep


def multi_quantize(items):
    """Multi-tensor K1: quantize many tensors (all weights of a model) in one launch per 32 tensors.

    items: iterable of (x, maxval, mbits[, n_bits[, sign_bits[, out]]]); every x on the same device.
    Returns the list of outputs (bit-identical to quantize() on each item)."""
    items = [tuple(it) for it in items]
    if not items:
        return []
    descs, outs, keep = _pack_descs(items)
    with _on_device(keep[0][0]):
        rc = lib().fp8q_multi_quantize_f32(descs, len(items), _stream(keep[0][0]))
    check(rc, "fp8q_multi_quantize_f32")
    return outs


def multi_minmax_quantize(items):
    """Multi-tensor K2+K5+K1: per-channel current_minmax ranges + quantize of many tensors in TWO launches
    (fp8q_multi_minmax_quantize_f32).  items: iterable of (x, maxval_out, mbits[, n_bits[, sign_bits[, out]]]);
    maxval_out is a [C] CUDA fp32 tensor that RECEIVES the ranges.  Returns the list of outputs (bit-identical to
    minmax_quantize() on each item)."""
    items = [tuple(it) for it in items]
    if not items:
        return []
    for it in items:
        if it[1].numel() != (it[0].shape[0] if it[0].dim() > 0 else 1) or not it[1].is_contiguous():
            raise Fp8qError("multi_minmax_quantize: maxval_out must be a contiguous [C] tensor")
    descs, outs, keep = _pack_descs(items)
    for (x, mv), it in zip(keep, items):
        if mv.data_ptr() != it[1].data_ptr():
            raise Fp8qError("multi_minmax_quantize: maxval_out must be contiguous (a copy would receive the ranges)")
    import ctypes
    mv_out = (ctypes.c_void_p * len(items))(*[mv.data_ptr() for _, mv in keep])      # where the ranges are WRITTEN
    with _on_device(keep[0][0]):
        rc = lib().fp8q_multi_minmax_quantize_f32(descs, mv_out, len(items), _stream(keep[0][0]))
    check(rc, "fp8q_multi_minmax_quantize_f32")
    return outs


def _pack_codec_descs(items, encode):
    """descriptors of (values-or-codes, maxval, mbits[, n_bits[, sign_bits[, out]]]) items for the multi-tensor codec:
    encode: x float32 -> out uint8; decode: x uint8 -> out float32.  Returns (descs, outs, keep)."""
    from ._lib import TensorDesc
    descs = (TensorDesc * len(items))()
    outs, keep = [], []
    src_dt, dst_dt = (torch.float32, torch.uint8) if encode else (torch.uint8, torch.float32)
    for d, it in zip(descs, items):
        x, maxval, mbits = it[0], it[1], it[2]
        n_bits = it[3] if len(it) > 3 else 8
        sign_bits = it[4] if len(it) > 4 else 1
        out = it[5] if len(it) > 5 else None
        _require(x, "x", src_dt)
        _require(maxval, "maxval", like=x)
        if keep and x.device != keep[0][0].device:
            raise Fp8qError("multi-tensor codec: all tensors must be on one device")
        x = x.contiguous()
        maxval = maxval.contiguous().view(-1)
        n_mv = maxval.numel()
        C, inner = _rows(x, n_mv != 1)
        if n_mv != 1 and n_mv != C:
            raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
        y = _out(out, x, dtype=dst_dt)
        d.x, d.y, d.maxval = x.data_ptr(), y.data_ptr(), maxval.data_ptr()
        d.C, d.inner, d.n_maxval = C, inner, n_mv
        d.mbits, d.n_bits, d.sign_bits = float(mbits), int(n_bits), int(sign_bits)
        outs.append(y)
        keep.append((x, maxval))
    return descs, outs, keep


def multi_minmax_encode(items):
    """Per-channel current_minmax ranges + storage codes of many tensors in TWO launches (fp8q_multi_minmax_encode_u8):
    items (x, maxval_out [C] (receives the ranges), mbits[, n_bits[, sign_bits[, out uint8]]]).  Returns the code tensors
    (bit-identical to encode(x, minmax(x, True).maxval) per item)."""
    import ctypes
    items = [tuple(it) for it in items]
    if not items:
        return []
    descs, outs, keep = _pack_codec_descs(items, True)
    for (x, mv), it in zip(keep, items):
        if mv.data_ptr() != it[1].data_ptr() or mv.numel() != (x.shape[0] if x.dim() > 0 else 1):
            raise Fp8qError("multi_minmax_encode: maxval_out must be a contiguous [C] tensor (it receives the ranges)")
    mv_out = (ctypes.c_void_p * len(items))(*[mv.data_ptr() for _, mv in keep])
    with _on_device(keep[0][0]):
        rc = lib().fp8q_multi_minmax_encode_u8(descs, mv_out, len(items), _stream(keep[0][0]))
    check(rc, "fp8q_multi_minmax_encode_u8")
    return outs


def multi_decode(items):
    """Storage codes of many tensors back to float32 in one launch per 32 tensors (fp8q_multi_decode_u8):
    items (codes uint8, maxval, mbits[, n_bits[, sign_bits[, out float32]]])."""
    items = [tuple(it) for it in items]
    if not items:
        return []
    descs, outs, keep = _pack_codec_descs(items, False)
    with _on_device(keep[0][0]):
        rc = lib().fp8q_multi_decode_u8(descs, len(items), _stream(keep[0][0]))
    check(rc, "fp8q_multi_decode_u8")
    return outs


_MULTI_MODES = {"quantize": 0, "encode": 3, "decode": 4}


def multi_route(items, mode="quantize"):
    """Which launch serves each tensor of a multi-tensor call (fp8q_multi_route, include/fp8q.h): host only, nothing is
    enqueued.  items: the tuples multi_quantize ("quantize": also multi_minmax_quantize and MultiPlan), multi_minmax_encode
    ("encode") or multi_decode ("decode") take -- pass `out` to have the real output's alignment decide.  Returns
    [(step, batched), ...] in item order: the launch the tensor lands in and whether that is the batched kernel (1) or
    the tensor's own single-tensor launch (0); (-1, -1) for an empty tensor."""
    import ctypes
    if mode not in _MULTI_MODES:
        raise Fp8qError(f"multi_route: mode must be one of {sorted(_MULTI_MODES)}, got {mode!r}")
    items = [tuple(it) for it in items]
    if not items:
        return []
    descs, _, _keep = _pack_descs(items) if mode == "quantize" else _pack_codec_descs(items, mode == "encode")
    n = len(items)
    step_of, batched, n_steps = (ctypes.c_int * n)(), (ctypes.c_int * n)(), ctypes.c_int()
    check(lib().fp8q_multi_route(descs, n, _MULTI_MODES[mode], step_of, batched, ctypes.byref(n_steps)), "fp8q_multi_route")
    return [(int(s), int(b)) for s, b in zip(step_of, batched)]


class MultiPlan:
    """Prepared multi-tensor K1 (fp8q_multi_plan_*): the descriptors of `items` are validated and packed once;
    launch() re-quantizes every tensor into its output with one ctypes call and one kernel launch per 32 tensors.
    The plan records addresses: it keeps the tensors alive, their contents may change between launches (in-place
    weight / range updates), their storage and shapes may not.  `outs` are the output tensors, in item order."""

    def __init__(self, items):
        import ctypes
        items = [tuple(it) for it in items]
        if not items:
            raise Fp8qError("MultiPlan needs at least one tensor")
        descs, self.outs, self._keep = _pack_descs(items)
        for (x, mv), it in zip(self._keep, items):
            if x.data_ptr() != it[0].data_ptr() or mv.data_ptr() != it[1].data_ptr():
                raise Fp8qError("MultiPlan needs contiguous tensors (a copy would be quantized instead of the tensor)")
        self._dev = self._keep[0][0]
        self._h = ctypes.c_void_p()
        check(lib().fp8q_multi_plan_create(descs, len(items), ctypes.byref(self._h)), "fp8q_multi_plan_create")
        self._launch = lib().fp8q_multi_plan_launch
        self._idx = self._dev.device.index

    @property
    def launches(self):
        return int(lib().fp8q_multi_plan_launches(self._h))

    def launch(self):
        if torch.cuda.current_device() != self._idx:
            with _on_device(self._dev):
                rc = self._launch(self._h, _stream(self._dev))
        else:
            rc = self._launch(self._h, _raw_stream(self._idx) if _raw_stream is not None else _stream(self._dev))
        if rc:
            check(rc, "fp8q_multi_plan_launch")
        return self.outs

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().fp8q_multi_plan_destroy(h)
            except Exception:
                pass


def new_packed(C, device):
    """[C, 4] fp32 buffer for the packed ranges of batch-sharded calibration (16-byte records)."""
    return torch.empty((C, 4), dtype=torch.float32, device=device)


def _check_packed(packed, C):
    _require(packed, "packed")
    if packed.numel() != 4 * C or not packed.is_contiguous() or packed.data_ptr() % 16:
        raise Fp8qError(f"packed must be a contiguous, 16-byte aligned [{C}, 4] tensor")


def ranges_unpack(packed, cur_min=None, cur_max=None, maxval=None):
    """After all-reduce(MAX) of a packed-ranges buffer (minmax(..., packed=) / affine_act_minmax(..., packed=)):
    cur_min / cur_max / maxval ([C] tensors, written in place; None = allocate).  Returns (cur_min, cur_max, maxval)."""
    _require(packed, "packed")
    n = packed.numel() // 4
    _check_packed(packed, n)
    if cur_min is None or cur_max is None or maxval is None:
        st = torch.empty((3, n), dtype=torch.float32, device=packed.device)
        cur_min = st[0] if cur_min is None else cur_min
        cur_max = st[1] if cur_max is None else cur_max
        maxval = st[2] if maxval is None else maxval
    for t in (cur_min, cur_max, maxval):
        _require(t, "range vector", like=packed)
        if t.numel() != n or not t.is_contiguous():
            raise Fp8qError("range vectors must be contiguous [C] tensors")
    with _on_device(packed):
        rc = lib().fp8q_ranges_unpack_f32(packed.data_ptr(), n, cur_min.data_ptr(), cur_max.data_ptr(),
                                          maxval.data_ptr(), _stream(packed))
    check(rc, "fp8q_ranges_unpack_f32")
    return cur_min, cur_max, maxval


def check_workspaces(clear=True):
    """SYNCHRONISES.  Inspect every min/max workspace this process has used since the last check -- the live ones and
    those a larger request has replaced in the meantime (fp8q_minmax_workspace_check): raises Fp8qError if a reducer
    block timed out (that call's range is NaN) or a workspace is dirty between calls.  Every workspace is inspected
    (and cleared) before the first failure is raised.  Called by QuantizedModel.fix_ranges(), i.e. once after
    calibration."""
    todo = [(k, w) for k, w in list(_ws_cache.items()) if k[2]] + list(_ws_retired)
    del _ws_retired[:]
    failures = []
    for (dev_index, stream, _zeroed, _kind), ws in todo:
        with torch.cuda.device(dev_index):
            rc = lib().fp8q_minmax_workspace_check(ws.data_ptr(), ws.numel(), int(bool(clear)), stream)
        if rc:
            failures.append(rc)
    if failures:
        check(failures[0], f"fp8q_minmax_workspace_check ({len(failures)} of {len(todo)} workspaces failed)")


def release_workspaces(keep_bytes=1 << 24, device=None):
    """Drop the scratch buffers larger than `keep_bytes` (the MSE search's partitioned keys: 4 B per element of the largest
    activation it has seen, ~300 MB for MobileNetV2 at batch 64) -- they are re-allocated on demand.  The zeroed min/max
    workspaces stay (small, and their headers carry state).  device: only that device's buffers (QuantizedModel.fix_ranges()
    passes its own device once calibration is over, so that another model still calibrating on another GPU of the process keeps
    its scratch); None: every device.  Streams are not told apart: a model calibrating on another stream of the SAME device
    re-allocates on its next batch.  Returns the bytes released."""
    idx = None if device is None else torch.device(device).index
    freed = 0
    for key, ws in list(_ws_cache.items()):
        if idx is not None and key[0] != idx:
            continue
        if not key[2] and key[3] in (None, "pre") and ws.numel() > keep_bytes:
            freed += ws.numel()
            del _ws_cache[key]
    return freed


def minmax(x, per_channel, cur_min=None, cur_max=None, mode=FOLD_CURRENT, momentum=0.9,
           want_maxval=False, packed=None):
    """K2/K3(/K5): batch min/max folded into the running estimate (range_estimators.py:61-125).

    cur_min/cur_max: running estimate tensors [C] (updated in place) or None on the first call.
    packed: optional [C, 4] buffer (new_packed) that receives {-min, max, nan flags} of the folded estimate for the
    range all-reduce of batch-sharded calibration (see ranges_unpack).
    x float16 / bfloat16: fp8q_minmax_h16 (estimates float32); no packed= buffer there.
    Returns (cur_min, cur_max[, maxval]) as [C] tensors.
    """
    half = isinstance(x, torch.Tensor) and x.dtype in _HALF
    if half and packed is not None:
        raise Fp8qError(f"packed ranges (data-parallel calibration) are float32-only, x is {x.dtype}")
    _require(x, "x", (torch.float32,) + _HALF)
    flat = None if per_channel else _dense_flat(x)      # per tensor: any dense layout, no copy
    x = flat if flat is not None else x.contiguous()
    C, inner = _rows(x, per_channel)
    if C == 0 or inner == 0:
        raise Fp8qError("min/max of an empty tensor")
    first = cur_min is None or cur_max is None
    mv = None
    if first:
        # one allocation for the two (three) result vectors: tiny tensors are host-bound, every torch.empty is ~2 us
        stats = torch.empty((3 if want_maxval else 2, C), dtype=torch.float32, device=x.device)
        if want_maxval:
            cur_min, cur_max, mv = stats.unbind(0)
        else:
            cur_min, cur_max = stats.unbind(0)
    else:
        _require(cur_min, "cur_min", like=x)
        _require(cur_max, "cur_max", like=x)
        if cur_min.numel() != C or cur_max.numel() != C or not cur_min.is_contiguous() \
                or not cur_max.is_contiguous():
            raise Fp8qError("running estimate has the wrong shape")
    if want_maxval and mv is None:
        mv = torch.empty(C, dtype=torch.float32, device=x.device)
    L = lib()
    nbytes = _mm_ws_bytes.get((C, inner))
    if nbytes is None:     # a pure function of the shape: one ctypes call per shape, not per launch
        nbytes = _mm_ws_bytes[(C, inner)] = L.fp8q_minmax_workspace_bytes(C, inner)
    ws = _workspace(x.device, nbytes, zeroed=True)
    if half:
        with _on_device(x):
            rc = L.fp8q_minmax_h16(x.data_ptr(), _DT[x.dtype], C, inner, cur_min.data_ptr(), cur_max.data_ptr(),
                                   mv.data_ptr() if mv is not None else None, int(mode), float(momentum),
                                   int(first), ws.data_ptr(), ws.numel(), _stream(x))
        check(rc, "fp8q_minmax_h16")
        return (cur_min, cur_max, mv) if want_maxval else (cur_min, cur_max)
    with _on_device(x):
        if packed is None:
            rc = L.fp8q_minmax_f32(x.data_ptr(), C, inner, cur_min.data_ptr(), cur_max.data_ptr(),
                                   mv.data_ptr() if mv is not None else None, int(mode), float(momentum),
                                   int(first), ws.data_ptr(), ws.numel(), _stream(x))
        else:
            _check_packed(packed, C)
            _require(packed, "packed", like=x)
            rc = L.fp8q_minmax_packed_f32(x.data_ptr(), C, inner, cur_min.data_ptr(), cur_max.data_ptr(),
                                          mv.data_ptr() if mv is not None else None, packed.data_ptr(), int(mode),
                                          float(momentum), int(first), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, "fp8q_minmax_f32")
    return (cur_min, cur_max, mv) if want_maxval else (cur_min, cur_max)


def fused_max_inner():
    return int(lib().fp8q_fused_max_inner())


ROWS_OPS = ("quantize", "minmax", "minmax_quantize")                 # FP8Q_ROWS_* (include/fp8q.h)
ROWS_KERNELS = ("k_quant_rows", "k_quant_scalar", "k_rows_flat", "k_rows_direct", "k_rows_reg", "k_rows_staged",
                "k_rows_staged_mm", "k_small_rows_fused", "k_minmax_partial")      # FP8Q_ROWS_K_*


def rows_route(op, C, inner, per_channel=True, mbits=2, n_bits=8, sign_bits=1, x_mod16=0, y_mod16=0, in_place=False):
    """The row kernel quantize / minmax / minmax_quantize (op, one of ROWS_OPS) reach for a [C, inner] float32 tensor of this
    format whose x and y sit at these addresses modulo 16 (fp8q_rows_route, include/fp8q.h), as a dict: kernel (a name of
    ROWS_KERNELS; None when nothing is launched), nontemporal, small, lut (bools), lanes, slots, group, nch, rows_per_block,
    nsplit, launches, grid_x, grid_y (of the first launch); what does not apply to the kernel is 0.  in_place: y is x.
    Host arithmetic only: needs no GPU.  Raises Fp8qError as the op's entry would for the shape."""
    import ctypes
    from ._lib import RowsRouteInfo
    info = RowsRouteInfo()
    check(lib().fp8q_rows_route(ROWS_OPS.index(op), int(C), int(inner), int(bool(per_channel)), float(mbits), int(n_bits),
                                int(sign_bits), int(x_mod16), int(x_mod16 if in_place else y_mod16), int(bool(in_place)),
                                ctypes.byref(info)), "fp8q_rows_route")
    r = {name: int(getattr(info, name)) for name, _ in RowsRouteInfo._fields_ if name != "reserved"}
    r["kernel"] = ROWS_KERNELS[info.kernel] if info.kernel >= 0 else None
    for name in ("nontemporal", "small", "lut"):
        r[name] = bool(r[name])
    return r


H16_KERNELS = ("k_h16_quant", "k_h16_quant_rows", "k_h16_minmax_rows", "k_h16_minmax_part")      # FP8Q_H16_K_*


def h16_route(op, C, inner, per_channel=True, mbits=2, n_bits=8, sign_bits=1, x_mod16=0, y_dtype=torch.float32):
    """The kernels quantize / minmax / minmax_quantize (op, one of ROWS_OPS) launch for a [C, inner] float16 / bfloat16 tensor
    whose x sits at this address modulo 16 (fp8q_h16_route, include/fp8q.h); y_dtype: float32 or x's own dtype (both half
    types take the same route).  A dict of the call's LAST kernel -- K1 for quantize and minmax_quantize, the scan for minmax:
    kernel (a name of H16_KERNELS), u, nontemporal (bool), head, groups, tail, rows_per_chunk, lds_bytes, lanes, nsplit, grid_x,
    grid_y, launches; what does not apply to the kernel is 0 -- plus "stages": the same dict for every kernel of the call in
    launch order (minmax_quantize: the scan, then K1).  Host arithmetic only: needs no GPU.  Raises Fp8qError as the op's
    entry would for the shape."""
    import ctypes
    from ._lib import H16LaunchInfo, H16RouteInfo
    info = H16RouteInfo()
    check(lib().fp8q_h16_route(ROWS_OPS.index(op), int(C), int(inner), int(bool(per_channel)), float(mbits), int(n_bits),
                               int(sign_bits), int(x_mod16), _DT[y_dtype], ctypes.byref(info)), "fp8q_h16_route")
    stages = []
    for k in range(info.n_launches):
        li = info.launch[k]
        d = {name: int(getattr(li, name)) for name, _ in H16LaunchInfo._fields_ if name != "reserved"}
        d["kernel"] = H16_KERNELS[li.kernel]
        d["nontemporal"] = bool(d["nontemporal"])
        stages.append(d)
    r = dict(stages[-1])
    r["stages"] = stages
    return r


_pct_ws_bytes = {}


def percentile_resident_max_inner():
    return int(lib().fp8q_percentile_resident_max_inner())


def percentile(x, per_channel, pct, lo=None, hi=None):
    """Percentile range of every row (range_estimators.py:61-70: np.percentile(x, (pct, 100 - pct))) by exact selection
    (fp8q_percentile_f32; contract: include/fp8q.h).  x: CUDA float32; returns (lo, hi), float32 [C] ([1] per tensor).
    lo= / hi=: contiguous float32 tensors of C elements to write into."""
    _require(x, "x")
    flat = None if per_channel else _dense_flat(x)      # per tensor: a multiset statistic, any dense layout, no copy
    x = flat if flat is not None else x.contiguous()
    C, inner = _rows(x, per_channel)
    if C == 0 or inner == 0:
        raise Fp8qError("percentile of an empty tensor")
    pct = float(pct)
    if lo is None or hi is None:
        fresh = torch.empty((2, C), dtype=torch.float32, device=x.device)
        lo, hi = (fresh[0] if lo is None else lo), (fresh[1] if hi is None else hi)
    for t, name in ((lo, "lo"), (hi, "hi")):
        _require(t, name, like=x)
        if t.numel() != C or not t.is_contiguous():
            raise Fp8qError(f"{name} must be a contiguous tensor of {C} elements (got {tuple(t.shape)})")
    L = lib()
    nbytes = _pct_ws_bytes.get((C, inner))
    if nbytes is None:
        nbytes = _pct_ws_bytes[(C, inner)] = L.fp8q_percentile_workspace_bytes(C, inner)
    stream = _stream(x)
    ws = _workspace(x.device, nbytes, stream=stream) if nbytes else None
    with _on_device(x):
        rc = L.fp8q_percentile_f32(x.data_ptr(), C, inner, pct, lo.data_ptr(), hi.data_ptr(),
                                   ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream)
    check(rc, "fp8q_percentile_f32")
    return lo, hi


def minmax_quantize(x, mbits, n_bits=8, sign_bits=1, out=None, out_dtype=None):
    """K2+K5+K1 fused per-channel weight quantization (current_minmax, set_maxval=True).
    x float16 / bfloat16 (fp8q_minmax_quantize_h16): y is float32 unless `out` / out_dtype=x.dtype ask for x's dtype.

    Returns (y, row_min, row_max, maxval)."""
    if isinstance(x, torch.Tensor) and x.dtype in _HALF:
        dt = _half_out_dtype(x, out, out_dtype)
        _require(x, "x", _HALF)
        x = x.contiguous()
        C, inner = _rows(x, True)
        y = _out(out, x, dtype=dt)
        mn, mx, mv = torch.empty((3, C), dtype=torch.float32, device=x.device).unbind(0)
        with _on_device(x):
            rc = lib().fp8q_minmax_quantize_h16(x.data_ptr(), y.data_ptr(), _DT[x.dtype], _DT[dt], C, inner, mn.data_ptr(),
                                                mx.data_ptr(), mv.data_ptr(), float(mbits), int(n_bits), int(sign_bits),
                                                _stream(x))
        check(rc, "fp8q_minmax_quantize_h16")
        return y, mn, mx, mv
    _require(x, "x")
    _check_out_dtype(x, out_dtype)
    x = x.contiguous()
    C, inner = _rows(x, True)
    y = _out(out, x)
    mn, mx, mv = torch.empty((3, C), dtype=torch.float32, device=x.device).unbind(0)   # one allocation (host-bound sizes)
    with _on_device(x):
        rc = lib().fp8q_minmax_quantize_f32(x.data_ptr(), y.data_ptr(), C, inner, mn.data_ptr(),
                                            mx.data_ptr(), mv.data_ptr(), float(mbits), int(n_bits),
                                            int(sign_bits), _stream(x))
    check(rc, "fp8q_minmax_quantize_f32")
    return y, mn, mx, mv


def _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n):
    """Checks of the INT entry points' range buffers: fp32 [n] delta (and zero_float, asymmetric), a 1-byte sign
    (symmetric: uint8 or bool), all contiguous on x's device.  Returns the three raw pointers (None where unused)."""
    bufs = [("delta", delta, torch.float32)]
    if symmetric:
        bufs.append(("signed_flag", signed_flag, (torch.uint8, torch.bool)))
    else:
        bufs.append(("zero_float", zero_float, torch.float32))
    for name, t, dt in bufs:
        _require(t, name, dt, like=x)
        if not t.is_contiguous() or t.numel() != (1 if name == "signed_flag" else n):
            raise Fp8qError(f"{name} must be a contiguous tensor of {1 if name == 'signed_flag' else n} elements")
    return (delta.data_ptr(), None if symmetric else zero_float.data_ptr(),
            signed_flag.data_ptr() if symmetric else None)


def _int_x(x, out, n_range, out_dtype=None, dense=False):
    """(x as the kernel reads it, y, C, inner, result): per tensor on a dense non-contiguous layout the storage as it
    lies (the result keeps x's strides, as the elementwise ATen chain does); otherwise a contiguous [C, inner] view.
    out_dtype: the result's dtype when it is not x's (integer codes: always the contiguous view, codes are storage;
    `dense`: values of a half input, which keep the layout)."""
    flat = _dense_flat(x) if (n_range == 1 and out is None and (out_dtype is None or dense)) else None
    if flat is not None:
        res = torch.empty_like(x, dtype=out_dtype)
        flat_out = _dense_flat(res) if res.stride() == x.stride() else None
        if flat_out is not None:
            return flat, flat_out, 1, flat.numel(), res
    x = x.contiguous()
    C, inner = _rows(x, n_range != 1)
    if n_range != 1 and n_range != C:
        raise Fp8qError(f"the range has {n_range} elements, expected 1 or {C}")
    y = _out(out, x, out_dtype)
    return x, y, C, inner, y


def _int_half(x, out, out_dtype):
    """The lane of an INT call by x's dtype: None for float32 x (out_dtype, when given, must be float32), the result's
    dtype for float16 / bfloat16 x (_half_out_dtype: float32 unless `out` / out_dtype ask for x's own).  Argument errors
    come before the device check: they need no GPU to be told."""
    if isinstance(x, torch.Tensor) and x.dtype in _HALF:
        dt = _half_out_dtype(x, out, out_dtype)
        _require(x, "x", _HALF)
        return dt
    if isinstance(x, torch.Tensor):
        _check_out_dtype(x, out_dtype)
    _require(x, "x")
    return None


def int_quantize(x, delta, zero_float=None, signed_flag=None, n_bits=8, symmetric=False, eps=1e-8, out=None,
                 out_dtype=None):
    """Uniform (INT) quantize+dequantize with fixed ranges (uniform_quantizers.py forward, linear scale domain):
    y = scale * (clamp(rint(x / scale) + zp, int_min, int_max) - zp).  delta (and zero_float, asymmetric) [1] or [C]
    CUDA fp32; symmetric: signed_flag is the quantizer's 1-byte device sign, read by the kernel.  One launch.
    x float16 / bfloat16 (fp8q_int_quantize_h16): x widened exactly, the fp32 chain, the result float32 unless `out` or
    out_dtype=x.dtype ask for x's own dtype (rounded once)."""
    dt = _int_half(x, out, out_dtype)
    delta = delta.detach().reshape(-1)
    n = delta.numel()
    zero_float = zero_float.detach().reshape(-1) if zero_float is not None else None
    signed_flag = signed_flag.detach().reshape(-1) if signed_flag is not None else None
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n)
    xk, y, C, inner, res = _int_x(x, out, n, dt, dense=True)
    if xk.numel() == 0:
        return res
    if dt is not None:
        with _on_device(xk):
            rc = lib().fp8q_int_quantize_h16(xk.data_ptr(), y.data_ptr(), _DT[x.dtype], _DT[dt], C, inner, pd, pz, n, ps,
                                             int(n_bits), int(bool(symmetric)), float(eps), _stream(xk))
        check(rc, "fp8q_int_quantize_h16")
        return res
    with _on_device(xk):
        rc = lib().fp8q_int_quantize_f32(xk.data_ptr(), y.data_ptr(), C, inner, pd, pz, n, ps, int(n_bits),
                                         int(bool(symmetric)), float(eps), _stream(xk))
    check(rc, "fp8q_int_quantize_f32")
    return res


def _int_code_dtype(n_bits):
    """storage dtype of the INT codes: one byte up to 8 bits, two from 9 to 16 (raw two's-complement bits)"""
    return torch.uint8 if int(n_bits) <= 8 else torch.int16


def _int_codec(fn, x, name, in_dtype, out_dtype, delta, zero_float, signed_flag, n_bits, symmetric, eps, out, half=None):
    """The launch shared by int_to_integer / int_encode / int_decode: int_quantize's checks, one kernel.  `half`: the
    float16 / bfloat16 side of an _h16 entry point, whose FP8Q_DT_* follows the two tensors."""
    _require(x, name, in_dtype)
    delta = delta.detach().reshape(-1)
    n = delta.numel()
    zero_float = zero_float.detach().reshape(-1) if zero_float is not None else None
    signed_flag = signed_flag.detach().reshape(-1) if signed_flag is not None else None
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n)
    xk, y, C, inner, res = _int_x(x, out, n, None if out_dtype is x.dtype else out_dtype)
    if xk.numel() == 0:
        return res
    types = () if half is None else (_DT[half],)
    _run(fn, xk, xk.data_ptr(), y.data_ptr(), *types, C, inner, pd, pz, n, ps, int(n_bits), int(bool(symmetric)), float(eps))
    return res


def int_to_integer(x, delta, zero_float=None, signed_flag=None, n_bits=8, symmetric=False, eps=1e-8, out=None):
    """The integer grid of int_quantize as float32 (uniform_quantizers.py to_integer_forward, linear scale domain):
    t = clamp(rint(x / scale) + zp, int_min, int_max), bit for bit the eager CUDA chain; NaN stays NaN, a zero level is +0
    (torch's CPU clamp keeps the -0 that -0 + -0 gives when zero_float is -0; its CUDA clamp does not).  Arguments as
    int_quantize.  One launch."""
    return _int_codec("fp8q_int_to_integer_f32", x, "x", torch.float32, torch.float32, delta, zero_float, signed_flag, n_bits,
                      symmetric, eps, out)


def int_encode(x, delta, zero_float=None, signed_flag=None, n_bits=8, symmetric=False, eps=1e-8, out=None):
    """The integers of int_quantize as storage codes, contiguous and shaped like x: torch.uint8 for n_bits <= 8, torch.int16
    for 9..16.  These are RAW two's-complement bits: `.view(torch.int8)` gives the integers of a signed symmetric quantizer
    (its codes of -2^(n-1) .. -1 read as 256 - |t| through uint8), and UNSIGNED 16-bit codes of 32768 and above read as
    negative numbers through int16 (add 65536, or widen and mask with 0xffff).  NaN inputs store the code of the value 0
    (zp, or 0 when symmetric).  int_decode(int_encode(x)) == int_quantize(x) bit for bit wherever x is not NaN.
    Arguments as int_quantize.  One launch.
    x float16 / bfloat16 (fp8q_int_encode_h16): x widened exactly, the same codes as int_encode(x.float())."""
    if isinstance(x, torch.Tensor) and x.dtype in _HALF:
        return _int_codec("fp8q_int_encode_h16", x, "x", _HALF, _int_code_dtype(n_bits), delta, zero_float, signed_flag,
                          n_bits, symmetric, eps, out, half=x.dtype)
    _require(x, "x", _VALUES)
    return _int_codec("fp8q_int_encode", x, "x", torch.float32, _int_code_dtype(n_bits), delta, zero_float, signed_flag, n_bits,
                      symmetric, eps, out)


def int_decode(codes, delta, zero_float=None, signed_flag=None, n_bits=8, symmetric=False, eps=1e-8, out=None,
               out_dtype=None):
    """Values of int_encode's codes (uint8 for n_bits <= 8, int16 for 9..16): y = scale * (code - zp), the code read as
    signed exactly when the quantizer is symmetric and its device sign flag is set.  float32 unless a float16 / bfloat16
    `out` or out_dtype asks for a half type (fp8q_int_decode_h16): the float32 value rounded once.  One launch."""
    dt = _decode_out_dtype(out, out_dtype)
    if dt in _HALF:
        return _int_codec("fp8q_int_decode_h16", codes, "codes", _int_code_dtype(n_bits), dt, delta, zero_float, signed_flag,
                          n_bits, symmetric, eps, out, half=dt)
    return _int_codec("fp8q_int_decode", codes, "codes", _int_code_dtype(n_bits), torch.float32, delta, zero_float,
                      signed_flag, n_bits, symmetric, eps, out)


def int_quantize_backward(x, g, delta, zero_float=None, signed_flag=None, n_bits=8, symmetric=False, eps=1e-8, need_gx=True,
                          need_gdelta=True, need_gzero=False, grad_scale_elems=0, out=None):
    """Backward of int_quantize (fp8q_int_quantize_bwd_f32): d/dx, d/ddelta and d/dzero_float for the upstream gradient g, in
    one pass over x and g -- the forward's integers are recomputed in the kernel, nothing but x and the ranges has to be kept.
    x, g: CUDA float32 of the same shape, contiguous (per tensor: any dense layout they share, as int_quantize()); the range
    arguments as int_quantize().  grad_scale_elems > 0: LSQ's gradient scaling, both range gradients times
    1 / sqrt(int_max * grad_scale_elems), int_max read on the device (numel / C per channel, numel per tensor).
    out (with need_gx): a contiguous CUDA float32 tensor of x's shape that receives gx.
    Returns (gx | None, gdelta | None, gzero_float | None): gx like x (or out), the others float32 [n_delta]."""
    _require(x, "x")
    _require(g, "g", like=x)
    if out is not None:
        _require(out, "out", like=x)
        if not need_gx or out.shape != x.shape or not out.is_contiguous():
            raise Fp8qError("out must be a contiguous tensor of x's shape, and only with need_gx")
    if g.shape != x.shape:
        raise Fp8qError(f"g has shape {tuple(g.shape)}, x {tuple(x.shape)}")
    if not (need_gx or need_gdelta or need_gzero):
        raise Fp8qError("int_quantize_backward: nothing requested")
    if need_gzero and symmetric:
        raise Fp8qError("int_quantize_backward: a symmetric quantizer has no zero_float")
    delta = delta.detach().reshape(-1)
    n = delta.numel()
    zero_float = zero_float.detach().reshape(-1) if zero_float is not None else None
    signed_flag = signed_flag.detach().reshape(-1) if signed_flag is not None else None
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n)
    x, g = x.detach(), g.detach()
    flat = _dense_flat(x) if (n == 1 and out is None and g.stride() == x.stride()) else None
    if flat is not None:
        # per tensor on a dense non-contiguous layout shared by x and g: the storage as it lies, gx keeps the strides
        res = torch.empty_like(x) if need_gx else None
        flat_out = _dense_flat(res) if (need_gx and res.stride() == x.stride()) else None
        if not need_gx or flat_out is not None:
            _, gd, gz = int_quantize_backward(flat, _dense_flat(g), delta, zero_float, signed_flag, n_bits, symmetric, eps,
                                              need_gx, need_gdelta, need_gzero, grad_scale_elems, out=flat_out)
            return res, gd, gz
    x, g = x.contiguous(), g.contiguous()
    C, inner = _rows(x, n != 1)
    if n != 1 and n != C:
        raise Fp8qError(f"the range has {n} elements, expected 1 or {C}")
    if x.numel() == 0:
        raise Fp8qError("int_quantize_backward of an empty tensor")
    gx = (out if out is not None else torch.empty_like(x)) if need_gx else None
    gd = torch.empty(n, dtype=torch.float32, device=x.device) if need_gdelta else None
    gz = torch.empty(n, dtype=torch.float32, device=x.device) if need_gzero else None
    L = lib()
    ws_ptr, ws_len = None, 0
    stream = _stream(x)
    if need_gdelta or need_gzero:
        nbytes = _bwd_ws_bytes.get(("int", C, inner, n))
        if nbytes is None:
            nbytes = _bwd_ws_bytes[("int", C, inner, n)] = L.fp8q_int_quantize_bwd_workspace_bytes(C, inner, n)
        ws = _workspace(x.device, nbytes, kind="grad", stream=stream)
        ws_ptr, ws_len = ws.data_ptr(), ws.numel()
    with _on_device(x):
        rc = L.fp8q_int_quantize_bwd_f32(x.data_ptr(), g.data_ptr(), gx.data_ptr() if need_gx else None, C, inner, pd, pz, n,
                                         ps, int(n_bits), int(bool(symmetric)), float(eps), int(grad_scale_elems),
                                         gd.data_ptr() if need_gdelta else None, gz.data_ptr() if need_gzero else None,
                                         ws_ptr, ws_len, stream)
    check(rc, "fp8q_int_quantize_bwd_f32")
    return gx, gd, gz


def _int_range_out(x_min, delta, zero_float, signed_flag, symmetric):
    n = x_min.numel()
    dev = x_min.device
    if delta is None:
        delta = torch.empty(x_min.shape, dtype=torch.float32, device=dev)
    if zero_float is None and not symmetric:
        zero_float = torch.empty(x_min.shape, dtype=torch.float32, device=dev)
    if signed_flag is None and symmetric:
        signed_flag = torch.empty((), dtype=torch.bool, device=dev)
    return n, delta, zero_float, signed_flag


def int_set_range(x_min, x_max, n_bits=8, symmetric=False, eps=1e-8, delta=None, zero_float=None, signed_flag=None):
    """set_quant_range of the uniform quantizers on the device: (x_min, x_max) [n] -> (delta, zero_float, signed_flag)
    (zero_float None when symmetric, signed_flag None when not).  Buffers passed in are written in place; missing
    ones are allocated with x_min's shape (signed_flag: a 0-dim bool).  One launch, no host round trip."""
    _require(x_min, "x_min")
    _require(x_max, "x_max", like=x_min)
    x_min, x_max = x_min.detach().contiguous(), x_max.detach().contiguous()
    if x_max.numel() != x_min.numel() or x_min.numel() == 0:
        raise Fp8qError("x_min and x_max must have the same, non-zero number of elements")
    n, delta, zero_float, signed_flag = _int_range_out(x_min, delta, zero_float, signed_flag, symmetric)
    pd, pz, ps = _int_ptrs(x_min, delta, zero_float, signed_flag, symmetric, n)
    with _on_device(x_min):
        rc = lib().fp8q_int_set_range_f32(x_min.data_ptr(), x_max.data_ptr(), n, pd, pz, ps, int(n_bits),
                                          int(bool(symmetric)), float(eps), _stream(x_min))
    check(rc, "fp8q_int_set_range_f32")
    return delta, zero_float, signed_flag


def int_range_quantize(x, x_min, x_max, n_bits=8, symmetric=False, eps=1e-8, delta=None, zero_float=None,
                       signed_flag=None, out=None, out_dtype=None):
    """int_set_range and int_quantize in ONE launch (the range-estimating forward).  Returns
    (y, delta, zero_float, signed_flag) like int_set_range.  x float16 / bfloat16 (fp8q_int_range_quantize_h16): y as
    int_quantize's, the ranges float32 as ever."""
    dt = _int_half(x, out, out_dtype)
    _require(x_min, "x_min", like=x)
    _require(x_max, "x_max", like=x)
    x_min, x_max = x_min.detach().contiguous(), x_max.detach().contiguous()
    if x_max.numel() != x_min.numel() or x_min.numel() == 0:
        raise Fp8qError("x_min and x_max must have the same, non-zero number of elements")
    n, delta, zero_float, signed_flag = _int_range_out(x_min, delta, zero_float, signed_flag, symmetric)
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n)
    xk, y, C, inner, res = _int_x(x, out, n, dt, dense=True)
    if xk.numel() == 0:
        return (res,) + int_set_range(x_min, x_max, n_bits, symmetric, eps, delta, zero_float, signed_flag)
    if dt is not None:
        with _on_device(xk):
            rc = lib().fp8q_int_range_quantize_h16(xk.data_ptr(), y.data_ptr(), _DT[x.dtype], _DT[dt], C, inner,
                                                   x_min.data_ptr(), x_max.data_ptr(), n, pd, pz, ps, int(n_bits),
                                                   int(bool(symmetric)), float(eps), _stream(xk))
        check(rc, "fp8q_int_range_quantize_h16")
        return res, delta, zero_float, signed_flag
    with _on_device(xk):
        rc = lib().fp8q_int_range_quantize_f32(xk.data_ptr(), y.data_ptr(), C, inner, x_min.data_ptr(),
                                               x_max.data_ptr(), n, pd, pz, ps, int(n_bits), int(bool(symmetric)),
                                               float(eps), _stream(xk))
    check(rc, "fp8q_int_range_quantize_f32")
    return res, delta, zero_float, signed_flag


def int_minmax_quantize(x, n_bits=8, symmetric=False, eps=1e-8, delta=None, zero_float=None, signed_flag=None,
                        out=None, out_dtype=None):
    """Per-channel current_minmax + set_quant_range + quantize of a uniform quantizer (weights): row min / max, then
    range and quantize in one more launch.  Returns (y, row_min, row_max, delta, zero_float, signed_flag).
    x float16 / bfloat16 (fp8q_int_minmax_quantize_h16): y as int_quantize's, row min / max and the ranges float32."""
    dt = _int_half(x, out, out_dtype)
    x = x.contiguous()
    C, inner = _rows(x, True)
    if C == 0 or inner == 0:
        raise Fp8qError("min/max of an empty tensor")
    y = _out(out, x, dt)
    mn, mx = torch.empty((2, C), dtype=torch.float32, device=x.device).unbind(0)
    n, delta, zero_float, signed_flag = _int_range_out(mn, delta, zero_float, signed_flag, symmetric)
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, n)
    L = lib()
    nbytes = _mm_ws_bytes.get((C, inner))
    if nbytes is None:
        nbytes = _mm_ws_bytes[(C, inner)] = L.fp8q_minmax_workspace_bytes(C, inner)
    ws = _workspace(x.device, nbytes, zeroed=True)
    if dt is not None:
        with _on_device(x):
            rc = L.fp8q_int_minmax_quantize_h16(x.data_ptr(), y.data_ptr(), _DT[x.dtype], _DT[dt], C, inner, mn.data_ptr(),
                                                mx.data_ptr(), pd, pz, ps, int(n_bits), int(bool(symmetric)), float(eps),
                                                ws.data_ptr(), ws.numel(), _stream(x))
        check(rc, "fp8q_int_minmax_quantize_h16")
        return y, mn, mx, delta, zero_float, signed_flag
    with _on_device(x):
        rc = L.fp8q_int_minmax_quantize_f32(x.data_ptr(), y.data_ptr(), C, inner, mn.data_ptr(), mx.data_ptr(), pd,
                                            pz, ps, int(n_bits), int(bool(symmetric)), float(eps), ws.data_ptr(),
                                            ws.numel(), _stream(x))
    check(rc, "fp8q_int_minmax_quantize_f32")
    return y, mn, mx, delta, zero_float, signed_flag


def int_sse_grid(x, per_channel, thr, n_bits=8, symmetric=True, one_sided=False, eps=1e-8, out=None):
    """LineSearchEstimator's candidates for a uniform quantizer in one pass: out[n_cand, C] (float64, updated in place;
    a zero-filled one when None) += row-sum of (x - q_k(x))^2, q_k the quantizer after
    set_quant_range(0 if one_sided else -thr[k, c], thr[k, c]).  x CUDA float32 or float64 (the float64 lane follows
    ATen's type promotion); thr CUDA fp32 [n_cand, C].  Two launches, no host round trip."""
    _require(x, "x", (torch.float32, torch.float64))
    _require(thr, "thr", like=x)
    x = x.contiguous()
    C, inner = _rows(x, per_channel)
    if C == 0 or inner == 0:
        raise Fp8qError("candidate search on an empty tensor")
    if thr.dim() != 2 or thr.shape[1] != C or thr.shape[0] == 0 or not thr.is_contiguous():
        raise Fp8qError(f"thr must be contiguous [n_cand, {C}]")
    n_cand = thr.shape[0]
    if out is None:
        out = torch.zeros((n_cand, C), dtype=torch.float64, device=x.device)
    else:
        _require(out, "out", torch.float64, like=x)
        if tuple(out.shape) != (n_cand, C) or not out.is_contiguous():
            raise Fp8qError(f"out must be contiguous [{n_cand}, {C}]")
    L = lib()
    ws = _workspace(x.device, L.fp8q_int_sse_grid_workspace_bytes(C, inner, n_cand))
    fn, name = ((L.fp8q_int_sse_grid_f64, "fp8q_int_sse_grid_f64") if x.dtype == torch.float64
                else (L.fp8q_int_sse_grid_f32, "fp8q_int_sse_grid_f32"))
    with _on_device(x):
        rc = fn(x.data_ptr(), C, inner, thr.data_ptr(), n_cand, int(n_bits), int(bool(symmetric)), int(bool(one_sided)),
                float(eps), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, name)
    return out


def copy(x, out=None):
    """float4 copy kernel with K1's launch shape (HBM ceiling yardstick)."""
    _require(x, "x")
    x = x.contiguous()
    y = _out(out, x)
    with _on_device(x):
        rc = lib().fp8q_copy_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream(x))
    check(rc, "fp8q_copy_f32")
    return y


_mse_ws_bytes = {}


def mse_grid(x, per_channel, grid, mbits_list, n_bits, sign_bits, mses):
    """K4: mses[n_m, n_cand, C] += row-mean((x - q(x; m, grid[i, c]))^2)  (range_estimators.py:337-347).

    grid: CUDA fp32 [n_cand, C]; mbits_list: python floats; mses: CUDA fp32, updated in place.
    A per-tensor call takes any dense layout as it lies (no NCHW copy).  The table then depends on the memory format in its
    last bits (~1e-7 relative): the lane-per-element routes add fp32 squares in storage order (the interval-histogram route's
    integer moments are order-free), so a near-tie between two candidates can fall differently for the same values in NCHW
    and in channels-last -- inside K4's stated contract (include/fp8q.h: 1e-5 per entry), as any other summation order is.
    """
    import ctypes
    _require(x, "x")
    _require(grid, "grid", like=x)
    _require(mses, "mses", like=x)
    flat = None if per_channel else _dense_flat(x)      # a per-tensor mean does not depend on the layout
    x = flat if flat is not None else x.contiguous()
    C, inner = _rows(x, per_channel)
    n_m = len(mbits_list)
    n_cand = grid.shape[0]
    if grid.dim() != 2 or grid.shape[1] != C or not grid.is_contiguous():
        raise Fp8qError(f"grid must be contiguous [n_cand, {C}]")
    if tuple(mses.shape) != (n_m, n_cand, C) or not mses.is_contiguous():
        raise Fp8qError(f"mses must be contiguous [{n_m}, {n_cand}, {C}]")
    L = lib()
    key = (C, inner, n_cand, n_m)
    nbytes = _mse_ws_bytes.get(key)
    if nbytes is None:     # a pure function of the shape: one ctypes call per shape, not per launch
        nbytes = _mse_ws_bytes[key] = L.fp8q_mse_workspace_bytes(C, inner, n_cand, n_m)
    ws = _workspace(x.device, nbytes)
    mb = (ctypes.c_float * n_m)(*[float(v) for v in mbits_list])
    with _on_device(x):
        rc = L.fp8q_mse_grid_f32(x.data_ptr(), C, inner, grid.data_ptr(), n_cand, mb, n_m, int(n_bits),
                                 int(sign_bits), mses.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, "fp8q_mse_grid_f32")
    return mses


def mse_route(C, inner, n_cand, mbits_list, n_bits=8, sign_bits=1):
    """The kernel mse_grid reaches for x [C, inner] with grid [n_cand, C] and these widths, and the choices its launcher takes
    from the shape (fp8q_mse_route, include/fp8q.h), as a dict: kernel (0 k_mse_grid, 1 k_mse_row, 2 the interval histogram),
    finish (0 none, 1 k_mse_final_tile, 2 k_mse_final), nsplit and, for the histogram, tiles_per_wg, part_wgs, slice_min,
    moments_threads, n_superblocks, top_scan.  Host arithmetic only: needs no GPU.  Raises Fp8qError as mse_grid would."""
    import ctypes
    from ._lib import MseRouteInfo
    n_m = len(mbits_list)
    mb = (ctypes.c_float * max(n_m, 1))(*[float(v) for v in mbits_list])
    info = MseRouteInfo()
    check(lib().fp8q_mse_route(int(C), int(inner), int(n_cand), mb, n_m, int(n_bits), int(sign_bits), ctypes.byref(info)),
          "fp8q_mse_route")
    return {name: int(getattr(info, name)) for name, _ in MseRouteInfo._fields_ if name != "reserved"}


_linspace_checked = {}     # (steps, fractions) -> True: the device kernel reproduces torch.linspace; False: host fall-back


def _linspace_self_check(steps, lo_frac, hi_frac, device):
    """Once per process and (steps, fractions): the device search-grid formula against torch.linspace itself on a few
    ranges -- the kernel hard-codes ATen's CPU evaluation (the steps / 2 split, one fused multiply-add per element),
    which another ATen build could do differently.  Synchronises (once).  Returns True when the device path may be used;
    on a mismatch the decision is cached and the search grids are made by torch.linspace on the host from then on
    (a host round trip per FIRST calibration batch of a quantizer -- slower, never wrong)."""
    key = (steps, lo_frac, hi_frac)
    ok = _linspace_checked.get(key)
    if ok is not None:
        return ok
    probe = torch.tensor([1.0, 0.7361, 3.3e-5, 123.456, 6.0e4, 0.0131, 2.5], dtype=torch.float32)
    got = torch.empty((steps, probe.numel()), dtype=torch.float32, device=device)
    dev_probe = probe.to(device)
    check(lib().fp8q_mse_linspace_f32(dev_probe.data_ptr(), probe.numel(), steps, lo_frac, hi_frac, got.data_ptr(),
                                      _stream(got)), "fp8q_mse_linspace_f32")
    want = torch.stack([torch.linspace(lo_frac * float(v), hi_frac * float(v), steps) for v in probe.tolist()], 1)
    ok = bool(torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)))
    if not ok:
        import warnings
        warnings.warn("fp8q_mse_linspace_f32 does not reproduce torch.linspace on this PyTorch build: the MSE search "
                      "grids are computed by torch.linspace on the host (one synchronisation per quantizer)")
    _linspace_checked[key] = ok
    return ok


def _linspace_host(mx, steps, lo_frac, hi_frac):
    """the reference's own construction (range_estimators.py:296-305), per channel, on the host"""
    vals = mx.detach().cpu().tolist()
    cols = [torch.linspace(lo_frac * float(v), hi_frac * float(v), steps) for v in vals]
    return torch.stack(cols, 1).contiguous().to(mx.device)


def mse_linspace(mx, steps=111, lo_frac=0.1, hi_frac=1.2):
    """[steps, C] float32 search grid of FP_MSE_Estimator on the device: column c == torch.linspace(lo_frac * mx[c],
    hi_frac * mx[c], steps), bit for bit (range_estimators.py:296-305) -- no host round trip."""
    _require(mx, "mx")
    mx = mx.contiguous().view(-1)
    C = mx.numel()
    if C == 0:
        return torch.empty((steps, 0), dtype=torch.float32, device=mx.device)
    with _on_device(mx):
        if not _linspace_self_check(int(steps), float(lo_frac), float(hi_frac), mx.device):
            return _linspace_host(mx, int(steps), float(lo_frac), float(hi_frac))
        grid = torch.empty((steps, C), dtype=torch.float32, device=mx.device)
        rc = lib().fp8q_mse_linspace_f32(mx.data_ptr(), C, int(steps), float(lo_frac), float(hi_frac), grid.data_ptr(),
                                         _stream(mx))
    check(rc, "fp8q_mse_linspace_f32")
    return grid


def minmax_linspace(x, per_channel, steps=111, lo_frac=0.1, hi_frac=1.2):
    """First calibration batch of FP_MSE_Estimator in ONE launch (fp8q_minmax_linspace_f32): row min / max, max|x| and
    the search grid of that maximum.  Returns (min [C], max [C], absmax [C], grid [steps, C])."""
    _require(x, "x")
    flat = None if per_channel else _dense_flat(x)
    x = flat if flat is not None else x.contiguous()
    C, inner = _rows(x, per_channel)
    if C == 0 or inner == 0:
        raise Fp8qError("min/max of an empty tensor")
    with _on_device(x):
        if not _linspace_self_check(int(steps), float(lo_frac), float(hi_frac), x.device):
            mn, mx, mv = minmax(x, per_channel, want_maxval=True)
            return mn, mx, mv, _linspace_host(mv, int(steps), float(lo_frac), float(hi_frac))
        stats = torch.empty((3 + int(steps), C), dtype=torch.float32, device=x.device)    # one allocation
        L = lib()
        nbytes = _mm_ws_bytes.get((C, inner))
        if nbytes is None:
            nbytes = _mm_ws_bytes[(C, inner)] = L.fp8q_minmax_workspace_bytes(C, inner)
        ws = _workspace(x.device, nbytes, zeroed=True)
        rc = L.fp8q_minmax_linspace_f32(x.data_ptr(), C, inner, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                                        stats[3].data_ptr(), int(steps), float(lo_frac), float(hi_frac), ws.data_ptr(),
                                        ws.numel(), _stream(x))
    check(rc, "fp8q_minmax_linspace_f32")
    return stats[0], stats[1], stats[2], stats[3:]


def mse_select(mses, grid, mbits_list, sign_bits=1):
    """Winner of the MSE grid search on the device (range_estimators.py:350-369): per channel the mantissa width with the
    smallest minimum, the plurality vote over the channels (torch.mode: smallest value on a tie), per channel the
    winning width's argmin candidate.  Returns (mbits [1] CUDA float32, vote index [1] CUDA int32, maxval [C],
    xmin [C] = -sign_bits * maxval) -- nothing comes back to the host."""
    import ctypes
    _require(mses, "mses")
    _require(grid, "grid", like=mses)
    n_m = len(mbits_list)
    if mses.dim() != 3 or mses.shape[0] != n_m or tuple(mses.shape[1:]) != tuple(grid.shape) or not mses.is_contiguous() \
            or not grid.is_contiguous():
        raise Fp8qError(f"mses must be contiguous [{n_m}, n_cand, C] and grid contiguous [n_cand, C]")
    n_cand, C = grid.shape
    dev = mses.device
    out = torch.empty((2, C), dtype=torch.float32, device=dev)
    mb = vote_slot(dev)                  # the device's vote arena: fix_ranges() brings every pending width over in one copy
    vote = torch.empty(1, dtype=torch.int32, device=dev)
    L = lib()
    ws = _workspace(dev, L.fp8q_mse_select_workspace_bytes(C, n_m), kind="select")     # (zero header: the last-workgroup ticket)
    mbh = (ctypes.c_float * n_m)(*[float(v) for v in mbits_list])
    with _on_device(mses):
        rc = L.fp8q_mse_select_f32(mses.data_ptr(), grid.data_ptr(), C, n_cand, mbh, n_m, int(sign_bits), mb.data_ptr(),
                                   vote.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream(mses))
    check(rc, "fp8q_mse_select_f32")
    return mb, vote, out[0], out[1]


# ---- mantissa-width votes: one arena per device --------------------------------------------------------------------------
# Every MSE estimator's voted width is a device scalar that the host wants exactly once, at fix_ranges().  Scalars that live
# in ONE buffer come over with one device-to-host copy (QuantizedModel.fix_ranges: materialize_mantissa_bits); gathering 116
# separately allocated scalars needed a torch.cat, whose kernel alone took 16 ms to load the first time a process used it.
_VOTE_SLOTS = 4096
_vote_arenas = {}      # device index -> [buffer, next free slot]
_vote_buffers = []     # every arena buffer still referenced by a view (weak): (weakref, base address)


def vote_slot(device):
    """A [1] float32 view into the device's vote arena (a fresh arena when the current one is full)."""
    import weakref
    ent = _vote_arenas.get(device.index)
    if ent is None or ent[1] >= _VOTE_SLOTS:
        buf = torch.zeros(_VOTE_SLOTS, dtype=torch.float32, device=device)
        ent = _vote_arenas[device.index] = [buf, 0]
        _vote_buffers[:] = [(r, a) for r, a in _vote_buffers if r() is not None]
        _vote_buffers.append((weakref.ref(buf), buf.data_ptr()))
    i = ent[1]
    ent[1] = i + 1
    return ent[0][i:i + 1]


def vote_arena_of(t):
    """(arena buffer, slot) if the 1-element CUDA float32 tensor t lies in a vote arena (vote_slot), else None.  By address:
    an arena's range belongs to it for as long as the buffer is alive, whatever chain of views / detach() led to t."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1):
        return None
    p = t.data_ptr()
    for r, addr in _vote_buffers:
        if addr <= p < addr + 4 * _VOTE_SLOTS:
            buf = r()
            if buf is not None and buf.device == t.device:
                return buf, (p - addr) // 4
    return None


_cal_ws_bytes = {}


class MseCalibration:
    """The persistent device state of one FP_MSE_Estimator and its quantizer, bound once, stepped with ONE library call per
    batch (fp8q_mse_calibrate_f32): abs-max + search grid (first batch), the MSE table of every (width, candidate), the
    vote / argmin, and the quantization of the batch with the winner -- QuantizationManager.forward in estimate state
    (quantization_manager.py:114-122 around range_estimators.py:318-369).  One allocation holds every result vector:
      block = [cur_min | cur_max | absmax | maxval | xmin] (5 C) | grid (n_cand C) | mses (n_m n_cand C) | vote (1, int32)
    The voted width lives in the device's vote arena (vote_slot)."""

    def __init__(self, C, device, mbits_list, n_bits, sign_bits, n_cand=111, grid=None, mses=None):
        import ctypes
        from ._lib import MseState
        self.C, self.n_cand, self.n_m = int(C), int(n_cand), len(mbits_list)
        self.n_bits, self.sign_bits = int(n_bits), int(sign_bits)
        self.mbits_list = [float(v) for v in mbits_list]
        C, n_m = self.C, self.n_m
        adopt = grid is not None and mses is not None
        n_tab = 0 if adopt else (n_cand * C + n_m * n_cand * C)
        blk = torch.empty(5 * C + n_tab + 1, dtype=torch.float32, device=device)
        self._blk = blk
        if adopt:           # tables made by the generic path (an earlier batch in another layout): keep accumulating into them
            _require(grid, "grid")
            _require(mses, "mses", like=grid)
            if tuple(grid.shape) != (n_cand, C) or tuple(mses.shape) != (n_m, n_cand, C) or not grid.is_contiguous() \
                    or not mses.is_contiguous() or grid.device != blk.device:
                raise Fp8qError("MseCalibration: grid / mses of the wrong shape")
            self.grid, self.mses = grid, mses
        else:
            self.grid = blk[5 * C:5 * C + n_cand * C].view(n_cand, C)
            self.mses = blk[5 * C + n_cand * C:5 * C + n_tab].view(n_m, n_cand, C)
        self.maxval = blk[3 * C:4 * C]
        self.mbits = vote_slot(blk.device)
        self.first = not adopt
        # (the other vectors of the block are views made on demand -- cur_min, cur_max, absmax, xmin, vote: a calibration pass
        # constructs 116 of these objects, every tensor view costs the host a microsecond or two)
        p0 = blk.data_ptr()
        self._state = MseState(p0, p0 + 4 * C, p0 + 8 * C, self.grid.data_ptr(), self.mses.data_ptr(), p0 + 12 * C, p0 + 16 * C,
                               self.mbits.data_ptr(), p0 + 4 * (5 * C + n_tab))
        self._sref = ctypes.byref(self._state)
        self._mb = (ctypes.c_float * n_m)(*self.mbits_list)
        self._fn = lib().fp8q_mse_calibrate_f32
        self._dev = blk.device
        self._idx = blk.device.index
        self._n_tab = n_tab

    cur_min = property(lambda self: self._blk[0:self.C])
    cur_max = property(lambda self: self._blk[self.C:2 * self.C])
    absmax = property(lambda self: self._blk[2 * self.C:3 * self.C])
    xmin = property(lambda self: self._blk[4 * self.C:5 * self.C])
    vote = property(lambda self: self._blk[5 * self.C + self._n_tab:].view(torch.int32))

    def _sizes(self, inner, pre_geo=None):
        import ctypes
        key = (self.C, inner, self.n_cand, self.n_m, pre_geo)
        sz = _cal_ws_bytes.get(key)
        if sz is None:
            a, b = ctypes.c_size_t(), ctypes.c_size_t()
            c = lib().fp8q_mse_calibrate_workspace_bytes(self.C, inner, self.n_cand, self.n_m, ctypes.byref(a), ctypes.byref(b))
            mm = int(a.value)
            if pre_geo is not None:
                mm = max(mm, int(lib().fp8q_affine_act_minmax_workspace_bytes(*pre_geo)))
            sz = _cal_ws_bytes[key] = (mm, int(b.value), int(c))
        return sz

    def step(self, x, quantize=True, pre=None):
        """x: contiguous CUDA float32 with C rows (per tensor: C == 1).  Returns the quantized batch (or None).
        pre = (bn_ab or None, residual or None, act): x is the PRODUCER's output [N, C, ...]; the search and the
        quantization run on act(bn(x) + residual), formed inside the same call (per-tensor quantizers only)."""
        inner = x.numel() // self.C
        dev = self._dev
        st = _raw_stream(self._idx) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
        pre_ref, keep = None, None
        xin = x
        if pre is not None:
            import ctypes
            from ._lib import AffinePre
            ab, res, act = pre
            N, C, HW = _nchw(x)
            if self.C != 1 or (ab is not None and (ab.numel() != 2 * C or not ab.is_contiguous() or ab.device != x.device)) \
                    or (res is not None and (res.shape != x.shape or not res.is_contiguous() or res.dtype != x.dtype
                                             or res.device != x.device)):
                raise Fp8qError("MseCalibration.step: bad `pre` (per-tensor quantizer, folded [C, 2] BN vector, residual like x)")
            mm, sel, mse = self._sizes(inner, (N, C, HW))
            t = _workspace(dev, 4 * inner, kind="pre", stream=st)   # the tensor the quantizer sees: scratch, consumed by this call
            keep = AffinePre(x.data_ptr(), res.data_ptr() if res is not None else None, ab.data_ptr() if ab is not None else None,
                             N, C, HW, int(act))
            pre_ref = ctypes.byref(keep)
            xin = t
        else:
            mm, sel, mse = self._sizes(inner)
        # (short per-channel rows need no min/max workspace: fp8q_minmax_workspace_bytes says 16 -- none is created then, so a
        # stream that only ever calibrates weights (QuantizedModel: calibrate_weights_ahead) owns no buffer that
        # check_workspaces() would have to synchronise for)
        ws_mm = _workspace(dev, mm, zeroed=True, stream=st) if (mm > 16 or self.C == 1) else None
        ws_sel = _workspace(dev, sel, kind="select", stream=st)
        ws_mse = _workspace(dev, mse, stream=st)
        y = torch.empty_like(x) if quantize else None
        first, self.first = self.first, False
        other = torch.cuda.current_device() != self._idx
        if other:
            prev = torch.cuda.current_device()
            torch.cuda.set_device(self._idx)
        try:
            rc = self._fn(xin.data_ptr(), y.data_ptr() if quantize else None, self.C, inner, self._sref, int(first), self.n_cand,
                          self._mb, self.n_m, self.n_bits, self.sign_bits, pre_ref, ws_mm.data_ptr() if ws_mm is not None else None,
                          ws_mm.numel() if ws_mm is not None else 0, ws_sel.data_ptr(),
                          ws_sel.numel(), ws_mse.data_ptr(), ws_mse.numel(), st)
        finally:
            if other:
                torch.cuda.set_device(prev)
        if rc:
            self.first = first
            check(rc, "fp8q_mse_calibrate_f32")
        return y


def minmax_f64(x, per_channel):
    """Row min / max of a float64 tensor as [C] float64 tensors (fp8q_minmax_f64): what LineSearchEstimator needs of
    its float64 sample (range_estimators.py:205-222: data.min(), data.max()).  NaN anywhere in a row -> NaN."""
    _require(x, "x", torch.float64)
    x = x.contiguous()
    C, inner = _rows(x, per_channel)
    if C == 0 or inner == 0:
        raise Fp8qError("min/max of an empty tensor")
    mn, mx = torch.empty((2, C), dtype=torch.float64, device=x.device).unbind(0)
    L = lib()
    ws = _workspace(x.device, L.fp8q_minmax_f64_workspace_bytes(C, inner))
    with _on_device(x):
        rc = L.fp8q_minmax_f64(x.data_ptr(), C, inner, mn.data_ptr(), mx.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, "fp8q_minmax_f64")
    return mn, mx


def mse_grid_f64(x, per_channel, grid, mbits_list, n_bits, sign_bits, out, reduce="sum"):
    """K4 on float64: out[n_m, n_cand, C] (float64, updated in place) += row-sum (reduce="sum": LineSearchEstimator.loss_fx,
    range_estimators.py:161-169) or row-mean (reduce="mean": FP_MSE_Estimator, :337-347) of (x - q(x; m, grid[i, c]))^2.
    grid: CUDA fp32 [n_cand, C] candidate maxvals (what torch.Tensor([x_max]) holds in the reference)."""
    import ctypes
    if reduce not in ("sum", "mean"):
        raise Fp8qError("reduce must be 'sum' or 'mean'")
    _require(x, "x", torch.float64)
    _require(grid, "grid", like=x)
    _require(out, "out", torch.float64, like=x)
    x = x.contiguous()
    C, inner = _rows(x, per_channel)
    n_m = len(mbits_list)
    n_cand = grid.shape[0]
    if grid.dim() != 2 or grid.shape[1] != C or not grid.is_contiguous():
        raise Fp8qError(f"grid must be contiguous [n_cand, {C}]")
    if tuple(out.shape) != (n_m, n_cand, C) or not out.is_contiguous():
        raise Fp8qError(f"out must be contiguous [{n_m}, {n_cand}, {C}]")
    L = lib()
    ws = _workspace(x.device, L.fp8q_mse_f64_workspace_bytes(C, inner, n_cand, n_m))
    mb = (ctypes.c_float * n_m)(*[float(v) for v in mbits_list])
    with _on_device(x):
        rc = L.fp8q_mse_grid_f64(x.data_ptr(), C, inner, grid.data_ptr(), n_cand, mb, n_m, int(n_bits), int(sign_bits),
                                 out.data_ptr(), int(reduce == "sum"), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, "fp8q_mse_grid_f64")
    return out


def encode(x, maxval, mbits, n_bits=8, sign_bits=1, out=None):
    """N3: uint8 storage codes of quantize(x) ([sign | exponent | fraction], fp8_quantizer.py:13-41).
    x float16 / bfloat16 (fp8q_encode_h16): x widened exactly, the same codes as encode(x.float())."""
    _require(x, "x", _VALUES)
    _require(maxval, "maxval", like=x)
    x = x.contiguous()
    maxval = maxval.contiguous().view(-1)
    n_mv = maxval.numel()
    C, inner = _rows(x, n_mv != 1)
    if n_mv != 1 and n_mv != C:
        raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
    codes = _out(out, x, torch.uint8)
    sfx, types = _lane(x.dtype, f32="_u8")
    if types and x.numel() == 0:      # (nothing to launch: fp8q_encode_u8 answers FP8Q_OK here, the _h16 entries refuse empty shapes)
        return codes
    _run("fp8q_encode" + sfx, x, x.data_ptr(), codes.data_ptr(), *types, C, inner, maxval.data_ptr(), n_mv, float(mbits),
         int(n_bits), int(sign_bits))
    return codes


def decode(codes, maxval, mbits, n_bits=8, sign_bits=1, out=None, out_dtype=None):
    """N3: values of uint8 storage codes; decode(encode(x)) == quantize(x) bit for bit when the channel's
    scale table is exactly geometric in fp32 (all weight-sized ranges), else within a few ULP (<= 5e-6 relative) on elements that round up
    into the next binade (see include/fp8q.h).  float32 unless a float16 / bfloat16 `out` or out_dtype asks for a half type
    (fp8q_decode_h16): the float32 value rounded once, so decode(encode(x), out_dtype=x.dtype) == quantize(x,
    out_dtype=x.dtype) under the same condition."""
    dt = _decode_out_dtype(out, out_dtype)
    if not isinstance(codes, torch.Tensor) or not codes.is_cuda or codes.dtype != torch.uint8:
        raise Fp8qError("codes must be a CUDA(HIP) uint8 tensor")
    _require(maxval, "maxval", like=codes)
    codes = codes.contiguous()
    maxval = maxval.contiguous().view(-1)
    n_mv = maxval.numel()
    C, inner = _rows(codes, n_mv != 1)
    if n_mv != 1 and n_mv != C:
        raise Fp8qError(f"maxval has {n_mv} elements, expected 1 or {C}")
    y = _out(out, codes, dt)
    sfx, types = _lane(dt, f32="_u8")
    if types and codes.numel() == 0:  # (as in encode: the same empty result as the float32 route)
        return y
    _run("fp8q_decode" + sfx, codes, codes.data_ptr(), y.data_ptr(), *types, C, inner, maxval.data_ptr(), n_mv, float(mbits),
         int(n_bits), int(sign_bits))
    return y


CODEC_KERNELS = ("k_rows_flat", "k_codec_rows")                      # FP8Q_CODEC_K_* (include/fp8q.h)


def codec_route(encode, C, inner, per_channel=True, mbits=2, n_bits=8, sign_bits=1, fp_mod16=0, code_mod16=0):
    """The kernel encode (encode true) / decode reach for a [C, inner] float32 tensor of this format whose float32 side and
    codes sit at these addresses modulo 16 (fp8q_codec_route, include/fp8q.h), as a dict: kernel (a name of CODEC_KERNELS; None
    when nothing is launched), nontemporal, wide (bools), nch, launches, grid_x, grid_y (of the first launch), steps; what does
    not apply to the kernel is 0.  Host arithmetic only: needs no GPU.  Raises Fp8qError as the entry would for the shape."""
    import ctypes
    from ._lib import CodecRouteInfo
    info = CodecRouteInfo()
    check(lib().fp8q_codec_route(int(bool(encode)), int(C), int(inner), int(C) if per_channel else 1, float(mbits), int(n_bits),
                                 int(sign_bits), int(fp_mod16), int(code_mod16), ctypes.byref(info)), "fp8q_codec_route")
    r = {name: int(getattr(info, name)) for name, _ in CodecRouteInfo._fields_ if name != "reserved"}
    r["kernel"] = CODEC_KERNELS[info.kernel] if info.kernel >= 0 else None
    for name in ("nontemporal", "wide"):
        r[name] = bool(r[name])
    return r


def chunk_route(C, inner, per_channel=True, elem_bytes=4, in_mod16=0, out_mod16=0, symmetric=False, sets_range=False):
    """The launch geometry of the chunked kernels -- the INT quantizers and codes, the hardware FP8 lane -- for a [C, inner]
    tensor of elem_bytes per element (4; 2: the INT kernels on half tensors) whose input and output sit at these addresses
    modulo 16 (fp8q_chunk_route, include/fp8q.h), as a dict: grid_x, rows_per_chunk, lds_bytes, magic, last_chunk (ints),
    per_channel, two_row, vec, nontemporal, sign_prepass (bools).  Host arithmetic only: needs no GPU.  Raises Fp8qError as
    the entries would for the shape."""
    import ctypes
    from ._lib import ChunkRouteInfo
    info = ChunkRouteInfo()
    check(lib().fp8q_chunk_route(int(C), int(inner), int(C) if per_channel else 1, int(elem_bytes), int(in_mod16),
                                 int(out_mod16), int(bool(symmetric)), int(bool(sets_range)), ctypes.byref(info)),
          "fp8q_chunk_route")
    r = {name: int(getattr(info, name)) for name, _ in ChunkRouteInfo._fields_ if name != "reserved"}
    for name in ("per_channel", "two_row", "vec", "nontemporal", "sign_prepass"):
        r[name] = bool(r[name])
    return r


# ---- hardware FP8: OCP E4M3FN / E5M2 (csrc/fp8q_ocp.hip; the contract is in include/fp8q.h) ----
_OCP_FMT = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}          # FP8Q_OCP_* (include/fp8q.h)
OCP_FMAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}


def _ocp_fmt(fmt):
    if fmt not in _OCP_FMT:
        raise Fp8qError(f"fmt must be torch.float8_e4m3fn or torch.float8_e5m2, got {fmt}")
    return _OCP_FMT[fmt]


def _ocp_range(t, name, like):
    """a range / scale vector as the kernels read it: float32, contiguous, flat, on `like`'s device"""
    _require(t, name, like=like)
    return t.detach().contiguous().view(-1)


def _ocp_rows(x, n):
    C, inner = _rows(x, n != 1)
    if n != 1 and n != C:
        raise Fp8qError(f"the range has {n} elements, expected 1 or {C}")
    return C, inner


def ocp_scale(maxval, fmt, eps=1e-8):
    """scale = max(maxval, eps) / fmax as the OCP kernels form it (fp8q_ocp_scale_f32), float32, shaped like maxval.flatten()"""
    f = _ocp_fmt(fmt)
    _require(maxval, "maxval")
    maxval = maxval.detach().contiguous().view(-1)
    scale = torch.empty_like(maxval)
    if maxval.numel():
        _run("fp8q_ocp_scale_f32", maxval, maxval.data_ptr(), maxval.numel(), f, float(eps), scale.data_ptr())
    return scale


def _ocp_sr(seed, offset):
    """(entry prefix suffix, trailing arguments) of an OCP call: ("", ()) for seed=None, ("sr", (seed, offset)) otherwise;
    checked as _mx_sr checks them, from the arguments alone, so raised before the device check"""
    sr = _mx_sr(seed, offset)
    return ("sr" if sr else ""), sr


def ocp_encode(x, maxval, fmt, eps=1e-8, out=None, want_scale=True, *, seed=None, offset=0):
    """Hardware FP8 codes of x: (codes, scale).  fmt: torch.float8_e4m3fn or torch.float8_e5m2; maxval [1] or [C] CUDA float32.
    scale = max(maxval, eps) / fmax, codes = RNE(clamp(x / scale, -fmax, fmax)) as OCP bytes -- what
    torch.clamp(x / scale, -fmax, fmax).to(fmt) gives on the CPU, every NaN as 0x7F.  codes is a tensor of dtype `fmt` shaped
    like x (a view of the uint8 buffer the kernel wrote; `out`: a contiguous uint8 or `fmt` tensor), scale float32 [1] or [C]
    (None with want_scale=False).  x float32, or float16 / bfloat16 (widened exactly: the codes of x.float()).  One launch.
    Dynamic scaling is minmax(x, per_channel, want_maxval=True) followed by this call.
    seed: None rounds to nearest even; a Python int in [0, 2^64) rounds stochastically, code = RNE(SR(q, r)) (include/fp8q.h:
    16 bits of Philox4x32-10 per element, drawn by the element's flat index offset + position in x as it lies; offset a
    multiple of 8), the draws of the mx_* ops: the same (seed, offset) gives the same draw to the same element in every
    ocp_* op, and a slice encoded under the same scale with the offset of its first element equals the slice of the whole."""
    f = _ocp_fmt(fmt)
    tag, sr = _ocp_sr(seed, offset)
    _require(x, "x", _VALUES)
    maxval = _ocp_range(maxval, "maxval", x)
    n = maxval.numel()
    x = x.contiguous()
    C, inner = _ocp_rows(x, n)
    if out is not None and isinstance(out, torch.Tensor) and out.dtype == fmt:
        out = out.view(torch.uint8)
    codes = _out(out, x, torch.uint8)
    scale = torch.empty_like(maxval) if want_scale else None
    if x.numel() == 0:
        return codes.view(fmt), (ocp_scale(maxval, fmt, eps) if want_scale else None)
    sfx, types = _lane(x.dtype)
    _run(f"fp8q_ocp{tag}_encode" + sfx, x, x.data_ptr(), codes.data_ptr(), *types, C, inner, maxval.data_ptr(), n, f,
         float(eps), scale.data_ptr() if want_scale else None, *sr)
    return codes.view(fmt), scale


def ocp_decode(codes, scale, out=None, out_dtype=None, fmt=None):
    """Values of hardware FP8 codes: value(code) * scale, one float32 multiplication -- codes.float() * scale of the CPU.
    codes: a CUDA tensor of dtype torch.float8_e4m3fn / torch.float8_e5m2, or uint8 with `fmt` naming the format; scale [1] or
    [C] CUDA float32 (ocp_encode's).  float32 unless a float16 / bfloat16 `out` or out_dtype asks for a half type (the float32
    product rounded once).  One launch."""
    dt = _decode_out_dtype(out, out_dtype)
    fmt = _codes_fmt(codes, fmt, _OCP_FMT, "float8_e4m3fn, float8_e5m2", "torch.float8_e4m3fn or torch.float8_e5m2")
    f = _ocp_fmt(fmt)
    scale = _ocp_range(scale, "scale", codes)
    n = scale.numel()
    codes = codes.contiguous().view(torch.uint8)
    C, inner = _ocp_rows(codes, n)
    y = _out(out, codes, dt)
    if codes.numel() == 0:
        return y
    sfx, types = _lane(dt)
    _run("fp8q_ocp_decode" + sfx, codes, codes.data_ptr(), y.data_ptr(), *types, C, inner, scale.data_ptr(), n, f)
    return y


def ocp_quantize(x, maxval, fmt, eps=1e-8, out=None, out_dtype=None, *, seed=None, offset=0):
    """Fake-quantize to hardware FP8: ocp_decode(*ocp_encode(x, maxval, fmt, eps)) bit for bit, in one launch.  x float32
    gives float32; x float16 / bfloat16 gives float32 unless `out` or out_dtype=x.dtype ask for x's own dtype (the float32
    result rounded once).  seed / offset: as in ocp_encode, and ocp_quantize(x, ..., seed=s) ==
    ocp_decode(*ocp_encode(x, ..., seed=s)) bit for bit."""
    f = _ocp_fmt(fmt)
    tag, sr = _ocp_sr(seed, offset)
    _require(x, "x", _VALUES)
    dt = _quantize_out_dtype(x, out, out_dtype)
    maxval = _ocp_range(maxval, "maxval", x)
    n = maxval.numel()
    x = x.contiguous()
    C, inner = _ocp_rows(x, n)
    y = _out(out, x, dt)
    if x.numel() == 0:
        return y
    sfx, types = _lane(x.dtype, dt)
    _run(f"fp8q_ocp{tag}_quantize" + sfx, x, x.data_ptr(), y.data_ptr(), *types, C, inner, maxval.data_ptr(), n, f,
         float(eps), *sr)
    return y


# ---- hardware FP8 under a float32 scale per tile (csrc/fp8q_ocp_block.hip; the contract is in include/fp8q.h) ----
OCP_BLOCK_TILES = ((1, 128), (128, 1), (128, 128))
OCP_BLOCK_KERNELS = ("rows", "panel", "plain")                     # FP8Q_OCPB_* (include/fp8q.h)


def _ocpb_tile(tile):
    try:
        t = tuple(tile)
    except TypeError:
        t = None
    if t not in OCP_BLOCK_TILES or any(isinstance(v, bool) for v in t):
        raise Fp8qError(f"tile must be (1, 128), (128, 1) or (128, 128), got {tile!r}")
    return t


def _ocpb_geometry(shape, tile):
    """(R, K, scales shape) of values shaped `shape` under `tile`: (1, 128) tiles the last dimension of any tensor (viewed as
    [-1, K]), the tiles that span rows need a matrix.  Told from the shape alone, so raised before the device check."""
    tr, tk = tile
    if len(shape) == 0:
        raise Fp8qError("the tiles run along the last dimension: the tensor needs at least one")
    if tr != 1 and len(shape) != 2:
        raise Fp8qError(f"{tr}x{tk} tiles span rows: x must be 2-D, got {len(shape)}-D {tuple(shape)} (reshape it to [R, K] "
                        f"first)")
    lead, K = tuple(int(s) for s in shape[:-1]), int(shape[-1])
    R = 1
    for s in lead:
        R *= s
    if tr == 1:
        return R, K, lead + (-(-K // tk),)
    return R, K, (-(-R // tr), -(-K // tk))


def ocp_block_route(R, K, tile, dtype, aligned16=True):
    """The kernel ocp_block_encode / ocp_block_quantize reach for an [R, K] tensor of `dtype` under `tile` -- fp8q_ocpb_route,
    the launchers' own rule, host arithmetic only (no GPU needed): "rows", "panel" or "plain".  aligned16: x and the output
    start on 16 bytes."""
    tr, tk = _ocpb_tile(tile)
    if dtype not in _DT:
        raise Fp8qError(f"dtype must be float32, float16 or bfloat16, got {dtype}")
    rc = lib().fp8q_ocpb_route(int(R), int(K), tr, tk, _DT[dtype], int(bool(aligned16)))
    if rc < 0:
        check(rc, "fp8q_ocpb_route")
    return OCP_BLOCK_KERNELS[rc]


def ocp_block_encode(x, fmt, tile=(1, 128), eps=1e-8, out=None, scales_out=None, *, seed=None, offset=0):
    """Block-scaled hardware FP8 operands of x: (codes, scales).  Every tile of `tile` = (1, 128), (128, 1) or (128, 128)
    elements gets its own float32 scale = max(amax(|tile|), eps) / fmax, found in the same pass; its codes are byte for byte
    ocp_encode(x[tile], amax, fmt, eps)'s.  codes: dtype `fmt`, x's shape and layout for every tile (nothing is transposed);
    scales: float32 [ceil(R / tr), ceil(K / tk)], row-major.  (1, 128) takes a tensor of any rank and tiles its last
    dimension (scales: x.shape[:-1] + (ceil(K / 128),)); the tiles that span rows need a 2-D x.  Edge tiles are short.  x
    float32, or float16 / bfloat16 (widened exactly).  `out`: contiguous uint8 or `fmt`; `scales_out`: contiguous float32 of
    the scales' shape.  One launch, x read once.  seed / offset: as in ocp_encode (the scales do not change)."""
    f = _ocp_fmt(fmt)
    tile = _ocpb_tile(tile)
    tag, sr = _ocp_sr(seed, offset)
    if isinstance(x, torch.Tensor):
        _ocpb_geometry(x.shape, tile)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    R, K, sshape = _ocpb_geometry(x.shape, tile)
    if out is not None and isinstance(out, torch.Tensor) and out.dtype == fmt:
        out = out.view(torch.uint8)
    codes = _out(out, x, torch.uint8)
    if scales_out is None:
        scales = torch.empty(sshape, dtype=torch.float32, device=x.device)
    else:
        _require(scales_out, "scales_out", like=x)
        if tuple(scales_out.shape) != sshape or not scales_out.is_contiguous():
            raise Fp8qError(f"scales_out must be a contiguous float32 tensor of shape {sshape}, got "
                            f"{tuple(scales_out.shape)}")
        scales = scales_out
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(f"fp8q_ocpb{tag}_encode" + sfx, x, x.data_ptr(), codes.data_ptr(), scales.data_ptr(), *types, R, K, *tile, f,
             float(eps), *sr)
    return codes.view(fmt).view(x.shape), scales


def ocp_block_decode(codes, scales, tile=(1, 128), out_dtype=None, out=None, fmt=None):
    """Values of block-scaled hardware FP8 operands: value(code) * scale of the element's tile, one float32 multiplication.
    codes: a CUDA tensor of dtype torch.float8_e4m3fn / torch.float8_e5m2, or uint8 with `fmt` naming the format; scales:
    float32, shaped as ocp_block_encode returns them for codes.shape and `tile`.  float32 unless a float16 / bfloat16 `out` or
    out_dtype asks for a half type (the float32 product rounded once).  One launch."""
    dt = _decode_out_dtype(out, out_dtype)
    tile = _ocpb_tile(tile)
    if isinstance(codes, torch.Tensor):
        _, _, sshape = _ocpb_geometry(codes.shape, tile)
        if isinstance(scales, torch.Tensor) and tuple(scales.shape) != sshape:
            raise Fp8qError(f"scales are {tuple(scales.shape)}, codes of shape {tuple(codes.shape)} under {tile} tiles have "
                            f"{sshape}")
    fmt = _codes_fmt(codes, fmt, _OCP_FMT, "float8_e4m3fn, float8_e5m2", "torch.float8_e4m3fn or torch.float8_e5m2")
    f = _ocp_fmt(fmt)
    _require(scales, "scales", like=codes)
    codes = codes.contiguous().view(torch.uint8)
    scales = scales.detach().contiguous()
    R, K, _ = _ocpb_geometry(codes.shape, tile)
    y = _out(out, codes, dt)
    if codes.numel() == 0:
        return y
    sfx, types = _lane(dt)
    _run("fp8q_ocpb_decode" + sfx, codes, codes.data_ptr(), scales.data_ptr(), y.data_ptr(), *types, R, K, *tile, f)
    return y


def ocp_block_quantize(x, fmt, tile=(1, 128), eps=1e-8, out_dtype=None, out=None, *, seed=None, offset=0):
    """Fake-quantize the way a block-scaled FP8 matrix multiplication sees x: ocp_block_decode(*ocp_block_encode(x, fmt,
    tile, eps), tile) bit for bit, in one launch, the scales never leaving the chip.  x float32 gives float32; x float16 /
    bfloat16 gives float32 unless `out` or out_dtype=x.dtype ask for x's own dtype (the float32 result rounded once).
    seed / offset: as in ocp_encode, and the identity above holds seed for seed."""
    f = _ocp_fmt(fmt)
    tile = _ocpb_tile(tile)
    tag, sr = _ocp_sr(seed, offset)
    if isinstance(x, torch.Tensor):
        _ocpb_geometry(x.shape, tile)
    _require(x, "x", _VALUES)
    dt = _quantize_out_dtype(x, out, out_dtype)
    x = x.detach().contiguous()
    R, K, _ = _ocpb_geometry(x.shape, tile)
    y = _out(out, x, dt)
    if x.numel() == 0:
        return y
    sfx, types = _lane(x.dtype, dt)
    _run(f"fp8q_ocpb{tag}_quantize" + sfx, x, x.data_ptr(), y.data_ptr(), *types, R, K, *tile, f, float(eps), *sr)
    return y


# ---- the same operands transposed: those of x.t(), from x as it lies (csrc/fp8q_ocp_block_t.hip) ----
OCP_BLOCK_T_TILES = ((1, 128), (128, 128))
OCP_BLOCK_T_KERNELS = ("panel", "plain")                            # FP8Q_OCPBT_* (include/fp8q.h)


def _ocpbt_tile(tile):
    t = _ocpb_tile(tile)
    if t not in OCP_BLOCK_T_TILES:
        raise Fp8qError(f"tile {t} has no transposed operands: they would be x's (1, 128) quantization with transposed codes, "
                        f"the operand of no product (the transposed tiles are (1, 128) and (128, 128); fake-quantization "
                        f"under column tiles is ocp_block_quantize(x, tile=(128, 1)))")
    return t


def _ocpbt_geometry(x, tile):
    """(R, K, row-wise scales shape, transposed scales shape) of a 2-D x; told from the shape alone, so raised before the
    device check"""
    if not isinstance(x, torch.Tensor):
        raise Fp8qError("x must be a CUDA(HIP) tensor: the FP8 engine has no CPU path")
    if x.dim() != 2:
        raise Fp8qError(f"the transposed operands are those of a matrix: x must be 2-D, got {x.dim()}-D {tuple(x.shape)} "
                        f"(reshape it to [R, K] first: the tiles are cut from that view's transpose)")
    R, K = int(x.shape[0]), int(x.shape[1])
    nR, nK = -(-R // 128), -(-K // 128)
    if tile == (1, 128):
        return R, K, (R, nK), (K, nR)
    return R, K, (nR, nK), (nK, nR)


def _ocpbt_buffer(out, name, dtypes, numel=None, shape=None):
    """the caller's `out`-style argument, checked from its metadata alone (before the device check): one of `dtypes`,
    contiguous, of `numel` elements (codes) or exactly `shape` (scales)"""
    if out is None:
        return
    want = " or ".join(str(d).replace("torch.", "") for d in dtypes)
    if not isinstance(out, torch.Tensor) or out.dtype not in dtypes:
        raise Fp8qError(f"{name} must be a {want} tensor, got {out.dtype if isinstance(out, torch.Tensor) else type(out)}")
    if shape is not None and tuple(out.shape) != tuple(shape):
        raise Fp8qError(f"{name} must be a contiguous {want} tensor of shape {tuple(shape)}, got {tuple(out.shape)}")
    if (numel is not None and out.numel() != numel) or not out.is_contiguous():
        raise Fp8qError(f"{name} must be a contiguous tensor of {numel if numel is not None else out.numel()} elements "
                        f"(got {tuple(out.shape)}, contiguous={out.is_contiguous()})")


def _ocpbt_take(out, name, shape, dtype, like):
    """a fresh tensor of `dtype` shaped `shape`, or the caller's (checked by _ocpbt_buffer) once it is on `like`'s device;
    codes as their uint8 view"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _require(out, name, out.dtype, like)
    return out.view(torch.uint8) if dtype == torch.uint8 else out


def ocp_block_t_route(R, K, tile, dtype, aligned16=True):
    """The kernel ocp_block_encode_t / ocp_block_encode_both reach for an [R, K] tensor of `dtype` under `tile` --
    fp8q_ocpbt_route, the launchers' own rule, host arithmetic only (no GPU needed).  aligned16: every tensor of the call
    starts on 16 bytes.  A dict: kernel "panel" or "plain", code_store_bytes (16, 4 or 1: the width of the transposed code
    stores), nontemporal."""
    from ._lib import OcpbtRouteInfo
    import ctypes
    tr, tk = _ocpbt_tile(tile)
    if dtype not in _DT:
        raise Fp8qError(f"dtype must be float32, float16 or bfloat16, got {dtype}")
    info = OcpbtRouteInfo()
    check(lib().fp8q_ocpbt_route(int(R), int(K), tr, tk, _DT[dtype], int(bool(aligned16)), ctypes.byref(info)),
          "fp8q_ocpbt_route")
    return {"kernel": OCP_BLOCK_T_KERNELS[info.kernel], "code_store_bytes": info.code_store_bytes,
            "nontemporal": bool(info.nontemporal)}


def ocp_block_encode_t(x, fmt, tile=(1, 128), eps=1e-8, out=None, scales_out=None, *, seed=None, offset=0):
    """Block-scaled hardware FP8 operands of x.t() made from x as it lies: (codes_t, scales_t), byte for byte
    ocp_block_encode(x.t().contiguous(), fmt, tile, eps) -- the operands of a product that reduces over dim 0 of x -- in one
    launch that reads x once and makes no transposed copy.  x: 2-D [R, K] (reshape anything else), float32 / float16 /
    bfloat16.  tile: (1, 128) or (128, 128).  codes_t: dtype `fmt`, [K, R]; scales_t: float32 [K, ceil(R / 128)] for
    (1, 128), [ceil(K / 128), ceil(R / 128)] for (128, 128).  ocp_block_decode(codes_t, scales_t, tile) gives the values of
    x.t().  `out`: contiguous uint8 or `fmt` of R * K elements; `scales_out`: contiguous float32 of the scales' shape.
    seed / offset: as in ocp_encode; an element is drawn by its position in x, not in x.t(), so with a seed this is NOT
    ocp_block_encode(x.t().contiguous(), ..., seed=seed) but the transposed half of ocp_block_encode_both(x, ..., seed=seed)."""
    f = _ocp_fmt(fmt)
    tile = _ocpbt_tile(tile)
    tag, sr = _ocp_sr(seed, offset)
    R, K, _, stshape = _ocpbt_geometry(x, tile)
    _ocpbt_buffer(out, "out", (torch.uint8, fmt), numel=R * K)
    _ocpbt_buffer(scales_out, "scales_out", (torch.float32,), shape=stshape)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    codes_t = _ocpbt_take(out, "out", (K, R), torch.uint8, x)
    scales_t = _ocpbt_take(scales_out, "scales_out", stshape, torch.float32, x)
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(f"fp8q_ocpbt{tag}_encode" + sfx, x, x.data_ptr(), codes_t.data_ptr(), scales_t.data_ptr(), *types, R, K, *tile, f,
             float(eps), *sr)
    return codes_t.view(fmt).view(K, R), scales_t


def ocp_block_encode_both(x, fmt, tile=(1, 128), eps=1e-8, out=None, scales_out=None, out_t=None, scales_out_t=None, *,
                          seed=None, offset=0):
    """Both orientations of x's block-scaled operands from ONE read of x: (codes, scales, codes_t, scales_t) =
    ocp_block_encode(x, fmt, tile, eps) + ocp_block_encode_t(x, fmt, tile, eps), byte for byte, in one launch.  (1, 128): two
    quantizations (row tiles and column tiles have their own scales); (128, 128): one, stored twice -- codes_t == codes.t()
    and scales_t == scales.t().  x: 2-D.  out / scales_out / out_t / scales_out_t: as in ocp_block_encode_t.  seed / offset: as
    in ocp_encode; both identities hold seed for seed."""
    f = _ocp_fmt(fmt)
    tile = _ocpbt_tile(tile)
    tag, sr = _ocp_sr(seed, offset)
    R, K, sshape, stshape = _ocpbt_geometry(x, tile)
    _ocpbt_buffer(out, "out", (torch.uint8, fmt), numel=R * K)
    _ocpbt_buffer(scales_out, "scales_out", (torch.float32,), shape=sshape)
    _ocpbt_buffer(out_t, "out_t", (torch.uint8, fmt), numel=R * K)
    _ocpbt_buffer(scales_out_t, "scales_out_t", (torch.float32,), shape=stshape)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    codes = _ocpbt_take(out, "out", (R, K), torch.uint8, x)
    scales = _ocpbt_take(scales_out, "scales_out", sshape, torch.float32, x)
    codes_t = _ocpbt_take(out_t, "out_t", (K, R), torch.uint8, x)
    scales_t = _ocpbt_take(scales_out_t, "scales_out_t", stshape, torch.float32, x)
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(f"fp8q_ocpbt{tag}_encode_both" + sfx, x, x.data_ptr(), codes.data_ptr(), scales.data_ptr(), codes_t.data_ptr(),
             scales_t.data_ptr(), *types, R, K, *tile, f, float(eps), *sr)
    return codes.view(fmt).view(R, K), scales, codes_t.view(fmt).view(K, R), scales_t


# ---- microscaling: blocks of 32 under an E8M0 scale byte (csrc/fp8q_mx.hip; the contract is in include/fp8q.h) ----
MX_E2M3, MX_E3M2 = "e2m3", "e3m2"      # the 6-bit formats: torch has no dtype for them, so strings name them and codes are uint8
_MX_FP6 = (MX_E2M3, MX_E3M2)
_MX_FMT = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1, torch.float4_e2m1fn_x2: 2, MX_E2M3: 4, MX_E3M2: 5}   # FP8Q_MX_* (include/fp8q.h; 3 is unassigned)
_MX_ROUNDING = {"floor": 0, "ceil": 1}
MX_BLOCK = 32
MX_SCALE_DTYPE = torch.float8_e8m0fnu


def _mx_fmt(fmt):
    if not isinstance(fmt, (torch.dtype, str)) or fmt not in _MX_FMT:
        raise Fp8qError(f"fmt must be torch.float8_e4m3fn, torch.float8_e5m2, torch.float4_e2m1fn_x2, 'e2m3' or 'e3m2', got {fmt!r}")
    return _MX_FMT[fmt]


def _mx_code_dtype(fmt):
    """the dtype codes of `fmt` are handed out as: the format's own, uint8 for the 6-bit formats"""
    return torch.uint8 if fmt in _MX_FP6 else fmt


def _mx_rounding(rounding):
    if rounding not in _MX_ROUNDING:
        raise Fp8qError(f"rounding must be 'floor' or 'ceil', got {rounding!r}")
    return _MX_ROUNDING[rounding]


def _mx_u64(v, name):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64:
        raise Fp8qError(f"{name} must be a Python int in [0, 2^64), got {v!r}")
    return v


def _mx_sr(seed, offset):
    """the trailing arguments of a stochastic-rounding entry, (seed, offset), or () for seed=None: round to nearest even, the
    entries without them.  Told from the arguments alone, so raised before the device check."""
    offset = _mx_u64(offset, "offset")
    if offset % 8:
        raise Fp8qError(f"offset must be a multiple of 8 (eight elements share one Philox call), got {offset}")
    if seed is None:
        if offset:
            raise Fp8qError(f"offset={offset} without a seed: round to nearest even draws nothing")
        return ()
    return (_mx_u64(seed, "seed"), offset)


def _mx_geometry(shape, fmt):
    """(lead, R, K, codes shape, scales shape) of values shaped `shape`: blocks run along the last dimension"""
    if len(shape) == 0:
        raise Fp8qError("MX blocks run along the last dimension: the tensor needs at least one")
    lead, K = tuple(shape[:-1]), int(shape[-1])
    R = 1
    for s in lead:
        R *= int(s)
    if fmt == torch.float4_e2m1fn_x2 and K % 2:
        raise Fp8qError(f"two E2M1 elements share a byte: the last dimension must be even, got {K}")
    if fmt in _MX_FP6 and K % 4:
        raise Fp8qError(f"four FP6 elements share three bytes: the last dimension must be a multiple of 4, got {K}")
    kc = K // 2 if fmt == torch.float4_e2m1fn_x2 else (3 * K // 4 if fmt in _MX_FP6 else K)
    return R, K, lead + (kc,), lead + ((K + MX_BLOCK - 1) // MX_BLOCK,)


def _mx_bytes(out, shape, dtype, name, like):
    """a uint8 view of a fresh tensor of `dtype` shaped `shape`, or of the caller's (uint8 or `dtype`, contiguous, as large)"""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=like.device)
    _require(out, name, (torch.uint8, dtype), like)
    n = 1
    for s in shape:
        n *= s
    if out.numel() != n or not out.is_contiguous():
        raise Fp8qError(f"{name} must be a contiguous tensor of {n} elements (got {tuple(out.shape)}, "
                        f"contiguous={out.is_contiguous()})")
    return out.view(torch.uint8)


def mx_encode(x, fmt, rounding="floor", out=None, scales_out=None, *, seed=None, offset=0):
    """MX operands of x: (codes, scales).  Blocks of 32 along the last dimension, one E8M0 scale byte each (include/fp8q.h
    states the arithmetic).  fmt: torch.float8_e4m3fn / torch.float8_e5m2 (codes shaped like x) or torch.float4_e2m1fn_x2
    (codes [..., K / 2], the even-indexed element in the low nibble; K must be even) or MX_E2M3 / MX_E3M2, the strings "e2m3" /
    "e3m2" (torch has no 6-bit dtype: codes are torch.uint8 [..., 3K / 4], four elements in three bytes, element i of a row
    in bits [6i, 6i + 6) of its little-endian bit string; K must be a multiple of 4).  scales: torch.float8_e8m0fnu
    [..., ceil(K / 32)].  rounding: "floor" (OCP MX v1.0: the largest elements of a block may saturate) or "ceil" (the smallest
    power of two under which none does).  x float32, or float16 / bfloat16 (widened exactly).  `out` / `scales_out`: contiguous
    tensors of the result's dtype or uint8.  One launch; the range is found in the same pass.
    seed: None rounds the elements to nearest even; a Python int in [0, 2^64) rounds them stochastically (include/fp8q.h: 16
    bits of Philox4x32-10 per element, drawn by the element's flat index offset + position in x -- so the same (seed, offset)
    gives the same draw to the same element in every mx_* op, and a slice encoded with the offset of its first element (a
    multiple of 8) equals the slice of the whole)."""
    f, r = _mx_fmt(fmt), _mx_rounding(rounding)
    sr = _mx_sr(seed, offset)
    if isinstance(x, torch.Tensor):
        _mx_geometry(x.shape, fmt)      # (argument errors before the device check: they need no GPU to be told)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    R, K, cshape, sshape = _mx_geometry(x.shape, fmt)
    cdt = _mx_code_dtype(fmt)
    codes = _mx_bytes(out, cshape, cdt, "out", x)
    scales = _mx_bytes(scales_out, sshape, MX_SCALE_DTYPE, "scales_out", x)
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(("fp8q_mxsr_encode" if sr else "fp8q_mx_encode") + sfx, x, x.data_ptr(), codes.data_ptr(), scales.data_ptr(),
             *types, R, K, f, r, *sr)
    return codes.view(cdt).view(cshape), scales.view(MX_SCALE_DTYPE).view(sshape)


def mx_decode(codes, scales, fmt=None, out_dtype=None, out=None):
    """Values of MX operands: value(elem) * 2^(scale - 127), one float32 multiplication; every element of a 0xFF block is NaN.
    codes: a CUDA tensor of an MX element dtype, or uint8 with `fmt` naming the format (the only way for "e2m3" / "e3m2", whose
    values have codes.shape[-1] * 4 / 3 elements in the last dimension); scales: torch.float8_e8m0fnu or uint8,
    one per block of 32 along the last dimension (mx_encode's).  float32 unless a float16 / bfloat16 `out` or out_dtype asks
    for a half type (the float32 product rounded once).  One launch."""
    dt = _decode_out_dtype(out, out_dtype)
    if isinstance(codes, torch.Tensor) and codes.dtype == torch.uint8:      # (argument errors before the device check)
        if fmt is None:
            raise Fp8qError("uint8 codes carry no format: pass fmt=")
        if fmt in _MX_FP6 and codes.dim() and codes.shape[-1] % 3:
            raise Fp8qError(f"four FP6 elements share three bytes: the codes' last dimension must be a multiple of 3, "
                            f"got {codes.shape[-1]}")
    fmt = _codes_fmt(codes, fmt, _MX_FMT, "float8_e4m3fn, float8_e5m2, float4_e2m1fn_x2", "")
    f = _mx_fmt(fmt)
    _require(scales, "scales", (MX_SCALE_DTYPE, torch.uint8), codes)
    if codes.dim() == 0:
        raise Fp8qError("MX blocks run along the last dimension: codes need at least one")
    codes = codes.contiguous().view(torch.uint8)
    kv = codes.shape[-1] * 4 // 3 if fmt in _MX_FP6 else codes.shape[-1] * (2 if fmt == torch.float4_e2m1fn_x2 else 1)
    vshape = tuple(codes.shape[:-1]) + (kv,)
    R, K, _, sshape = _mx_geometry(vshape, fmt)
    scales = scales.contiguous().view(torch.uint8)
    if tuple(scales.shape) != sshape:
        raise Fp8qError(f"scales are {tuple(scales.shape)}, values of shape {vshape} have {sshape}")
    if out is None:
        y = torch.empty(vshape, dtype=dt, device=codes.device)
    else:
        _require(out, "out", dt, codes)
        if out.numel() != R * K or not out.is_contiguous():
            raise Fp8qError(f"out must be a contiguous tensor of {R * K} elements (got {tuple(out.shape)}, "
                            f"contiguous={out.is_contiguous()})")
        y = out
    if R * K == 0:
        return y
    sfx, types = _lane(dt)
    _run("fp8q_mx_decode" + sfx, codes, codes.data_ptr(), scales.data_ptr(), y.data_ptr(), *types, R, K, f)
    return y


def mx_quantize(x, fmt, rounding="floor", out_dtype=None, out=None, *, seed=None, offset=0):
    """Fake-quantize the way an MX matrix multiplication sees x: mx_decode(*mx_encode(x, fmt, rounding)) bit for bit, in one
    launch, the scales never leaving the registers.  x float32 gives float32; x float16 / bfloat16 gives float32 unless `out`
    or out_dtype=x.dtype ask for x's own dtype (the float32 result rounded once).  seed / offset: as in mx_encode, and
    mx_quantize(x, seed=s) == mx_decode(*mx_encode(x, seed=s)) bit for bit."""
    f, r = _mx_fmt(fmt), _mx_rounding(rounding)
    sr = _mx_sr(seed, offset)
    if isinstance(x, torch.Tensor):
        _mx_geometry(x.shape, fmt)      # (argument errors before the device check, as in mx_encode)
    _require(x, "x", _VALUES)
    dt = _quantize_out_dtype(x, out, out_dtype)
    x = x.detach().contiguous()
    R, K, _, _ = _mx_geometry(x.shape, fmt)
    y = _out(out, x, dt)
    if x.numel() == 0:
        return y
    sfx, types = _lane(x.dtype, dt)
    _run(("fp8q_mxsr_quantize" if sr else "fp8q_mx_quantize") + sfx, x, x.data_ptr(), y.data_ptr(), *types, R, K, f, r, *sr)
    return y


# ---- microscaling with the blocks along dim 0: the operands of x.t() from x as it lies (csrc/fp8q_mx_t.hip) ----
def _mx_t_geometry(x, fmt, need_r=True, need_k=False):
    """(R, K) of a 2-D x whose MX blocks run along dim 0; need_r / need_k: the packing of codes along R / K must come out in
    whole bytes (the encoders).  Everything here is told from the shape alone, so it is raised before the device check."""
    if not isinstance(x, torch.Tensor):
        raise Fp8qError("x must be a CUDA(HIP) tensor: the FP8 engine has no CPU path")
    if x.dim() != 2:
        raise Fp8qError(f"the transposed MX operands are those of a matrix: x must be 2-D, got {x.dim()}-D {tuple(x.shape)} "
                        f"(reshape it to [R, K] first: the blocks run along dim 0 of that view)")
    R, K = int(x.shape[0]), int(x.shape[1])
    for need, n, what in ((need_r, R, "dim 0 (rows)"), (need_k, K, "the last dimension")):
        if need and fmt == torch.float4_e2m1fn_x2 and n % 2:
            raise Fp8qError(f"two E2M1 elements share a byte: {what} must be even, got {n}")
        if need and fmt in _MX_FP6 and n % 4:
            raise Fp8qError(f"four FP6 elements share three bytes: {what} must be a multiple of 4, got {n}")
    return R, K


def mx_t_route(R, K, fmt, dtype, aligned16=True):
    """The kernel mx_encode_t / mx_encode_both / mx_quantize_t reach for an [R, K] tensor of `dtype` -- fp8q_mxt_route, the
    launchers' own rule, host arithmetic only (no GPU needed).  aligned16: every tensor of the call starts on 16 bytes.
    A dict: kernel "tile" or "general", tile_rows / tile_cols (the tile kernel's), nontemporal, code_store_bytes."""
    from ._lib import MxtRouteInfo
    import ctypes
    if dtype not in _DT:
        raise Fp8qError(f"dtype must be float32, float16 or bfloat16, got {dtype}")
    info = MxtRouteInfo()
    check(lib().fp8q_mxt_route(int(R), int(K), _mx_fmt(fmt), _DT[dtype], int(bool(aligned16)), ctypes.byref(info)),
          "fp8q_mxt_route")
    return {"kernel": "tile" if info.kernel == 0 else "general", "tile_rows": info.tile_rows, "tile_cols": info.tile_cols,
            "nontemporal": bool(info.nontemporal), "code_store_bytes": info.code_store_bytes}


def mx_encode_t(x, fmt, rounding="floor", out=None, scales_out=None, *, seed=None, offset=0):
    """MX operands of x.t() made from x as it lies: (codes_t, scales_t), byte for byte mx_encode(x.t().contiguous(), fmt,
    rounding) -- blocks of 32 along dim 0 of x, for a product that reduces over it -- in one launch that reads x once and
    makes no transposed copy.  x: 2-D [R, K] (reshape anything else), float32 / float16 / bfloat16.  codes_t: [K, R] (FP8),
    [K, R / 2] (E2M1: rows 2i and 2i + 1 of a column share a byte, R even) or uint8 [K, 3R / 4] ("e2m3" / "e3m2": R a multiple
    of 4); scales_t: torch.float8_e8m0fnu [K, ceil(R / 32)].  mx_decode(codes_t, scales_t).t() gives the values back.
    seed / offset: as in mx_encode; the draws go by the position in x, not in x.t()."""
    f, r = _mx_fmt(fmt), _mx_rounding(rounding)
    sr = _mx_sr(seed, offset)
    _mx_t_geometry(x, fmt)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    R, K = x.shape
    _, _, cshape, sshape = _mx_geometry((K, R), fmt)
    cdt = _mx_code_dtype(fmt)
    codes = _mx_bytes(out, cshape, cdt, "out", x)
    scales = _mx_bytes(scales_out, sshape, MX_SCALE_DTYPE, "scales_out", x)
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(("fp8q_mxsr_encode_t" if sr else "fp8q_mxt_encode") + sfx, x, x.data_ptr(), codes.data_ptr(), scales.data_ptr(),
             *types, R, K, f, r, *sr)
    return codes.view(cdt).view(cshape), scales.view(MX_SCALE_DTYPE).view(sshape)


def mx_encode_both(x, fmt, rounding="floor", out=None, scales_out=None, out_t=None, scales_out_t=None, *, seed=None,
                   offset=0):
    """Both orientations of x's MX operands from ONE read of x: (codes, scales, codes_t, scales_t) = mx_encode(x) +
    mx_encode_t(x), byte for byte, in one launch.  x: 2-D; E2M1 needs R and K even, the 6-bit formats multiples of 4.
    out / scales_out / out_t / scales_out_t: contiguous tensors of the results' dtype or uint8, as in mx_encode.
    seed / offset: as in mx_encode; an element has one draw, used by both orientations."""
    f, r = _mx_fmt(fmt), _mx_rounding(rounding)
    sr = _mx_sr(seed, offset)
    _mx_t_geometry(x, fmt, need_k=True)
    _require(x, "x", _VALUES)
    x = x.detach().contiguous()
    R, K = x.shape
    _, _, cshape, sshape = _mx_geometry((R, K), fmt)
    _, _, ctshape, stshape = _mx_geometry((K, R), fmt)
    cdt = _mx_code_dtype(fmt)
    codes = _mx_bytes(out, cshape, cdt, "out", x)
    scales = _mx_bytes(scales_out, sshape, MX_SCALE_DTYPE, "scales_out", x)
    codes_t = _mx_bytes(out_t, ctshape, cdt, "out_t", x)
    scales_t = _mx_bytes(scales_out_t, stshape, MX_SCALE_DTYPE, "scales_out_t", x)
    if x.numel():
        sfx, types = _lane(x.dtype)
        _run(("fp8q_mxsr_encode_both" if sr else "fp8q_mxt_encode_both") + sfx, x, x.data_ptr(), codes.data_ptr(),
             scales.data_ptr(), codes_t.data_ptr(), scales_t.data_ptr(), *types, R, K, f, r, *sr)
    return (codes.view(cdt).view(cshape), scales.view(MX_SCALE_DTYPE).view(sshape),
            codes_t.view(cdt).view(ctshape), scales_t.view(MX_SCALE_DTYPE).view(stshape))


def mx_quantize_t(x, fmt, rounding="floor", out_dtype=None, out=None, *, seed=None, offset=0):
    """Fake-quantize x with the MX blocks along dim 0, in x's own layout: mx_decode(*mx_encode_t(x, fmt, rounding)).t() bit
    for bit, in one launch.  x: 2-D, any R and K -- nothing is packed, so E2M1 and the 6-bit formats need no divisible shape
    here (mx_encode_t does).  Output dtype as mx_quantize.  seed / offset: as in mx_encode_t."""
    f, r = _mx_fmt(fmt), _mx_rounding(rounding)
    sr = _mx_sr(seed, offset)
    _mx_t_geometry(x, fmt, need_r=False)
    _require(x, "x", _VALUES)
    dt = _quantize_out_dtype(x, out, out_dtype)
    x = x.detach().contiguous()
    R, K = x.shape
    y = _out(out, x, dt)
    if x.numel() == 0:
        return y
    sfx, types = _lane(x.dtype, dt)
    _run(("fp8q_mxsr_quantize_t" if sr else "fp8q_mxt_quantize") + sfx, x, x.data_ptr(), y.data_ptr(), *types, R, K, f, r, *sr)
    return y


def _nchw(x):
    """[N, C, *spatial] -> (N, C, HW)."""
    if x.dim() < 2:
        raise Fp8qError("fused epilogue expects [N, C, ...] tensors")
    N, C = x.shape[0], x.shape[1]
    return N, C, (x.numel() // (N * C) if N * C else 0)


def _bn_ptrs(bn, C, dev):
    if bn is None:
        return (None, None, None, None), ()
    keep = []
    for t in bn:
        _require(t, "bn parameter")
        t = t.contiguous()
        if t.numel() != C or t.device != dev:
            raise Fp8qError("batch-norm vectors must be [C] tensors on x's device")
        keep.append(t)
    return tuple(t.data_ptr() for t in keep), tuple(keep)


def affine_act_supported(x):
    """fp8q_affine_act_* needs C*HW % 4 == 0 (16-byte groups never straddle images)."""
    N, C, HW = _nchw(x)
    return N > 0 and (C * HW) % 4 == 0 and x.data_ptr() % 16 == 0


def bn_fold(bn):
    """[C, 2] fp32 {alpha, beta'} = {invstd * gamma, fma(-mean, alpha, beta)} of an eval-mode batch norm
    (fp8q_bn_fold_f32): the per-channel constants of the fused epilogue, folded once per parameter set."""
    mean = bn[0]
    _require(mean, "bn parameter")
    C = mean.numel()
    ptrs, keep = _bn_ptrs(bn, C, mean.device)
    ab = torch.empty((C, 2), dtype=torch.float32, device=mean.device)
    with _on_device(mean):
        rc = lib().fp8q_bn_fold_f32(ptrs[0], ptrs[1], ptrs[2], ptrs[3], C, ab.data_ptr(), _stream(mean))
    check(rc, "fp8q_bn_fold_f32")
    return ab


PREP_FLOATS = 264      # FP8Q_PREP_BYTES / 4


def quantizer_prepare(maxval, mbits, n_bits=8, sign_bits=1):
    """[264] fp32 block of a FIXED-range per-tensor quantizer: its channel constants and {s, 1/s} table, as the fused
    epilogue rebuilds them from maxval on every launch (fp8q_quantizer_prepare_f32).  Pass as affine_act_quantize(prep=)."""
    _require(maxval, "maxval")
    if maxval.numel() != 1:
        raise Fp8qError("quantizer_prepare: per-tensor quantizers only (one maxval)")
    prep = torch.empty(PREP_FLOATS, dtype=torch.float32, device=maxval.device)
    with _on_device(maxval):
        rc = lib().fp8q_quantizer_prepare_f32(maxval.contiguous().data_ptr(), float(mbits), int(n_bits), int(sign_bits),
                                              prep.data_ptr(), _stream(maxval))
    check(rc, "fp8q_quantizer_prepare_f32")
    return prep


def affine_act_quantize(x, maxval, mbits, n_bits=8, sign_bits=1, bn=None, residual=None, act=0, out=None, bn_ab=None,
                        prep=None):
    """N2: quantize(act(bn(x) + residual)) in one pass.  bn = (mean, invstd, gamma, beta), each [C] -- or bn_ab = the
    folded [C, 2] vector of bn_fold(bn) (same result, fewer loads); act: 0 none, 1 ReLU, 2 ReLU6; per-tensor maxval [1];
    prep = quantizer_prepare(maxval, mbits, n_bits, sign_bits) of the SAME quantizer (fixed ranges: the table is not rebuilt)."""
    _require(x, "x")
    _require(maxval, "maxval", like=x)
    x = x.contiguous()
    N, C, HW = _nchw(x)
    if residual is not None:
        _require(residual, "residual", like=x)
        residual = residual.contiguous()
        if residual.shape != x.shape:
            raise Fp8qError("residual must have x's shape")
    if maxval.numel() != 1:
        raise Fp8qError("the fused epilogue quantizes per tensor: maxval must have one element")
    y = _out(out, x)
    if prep is not None:
        _require(prep, "prep", like=x)
        if prep.numel() != PREP_FLOATS or not prep.is_contiguous() or prep.data_ptr() % 16:
            raise Fp8qError("prep must be the [264] fp32 block of fp8q.ops.quantizer_prepare")
    if bn_ab is not None or (prep is not None and bn is None):
        if bn_ab is not None:
            _require(bn_ab, "bn_ab", like=x)
            if bn_ab.numel() != 2 * C or not bn_ab.is_contiguous():
                raise Fp8qError("bn_ab must be a contiguous [C, 2] tensor (fp8q.ops.bn_fold)")
        with _on_device(x):
            rc = lib().fp8q_affine_act_quantize_ab_f32(
                x.data_ptr(), residual.data_ptr() if residual is not None else None, y.data_ptr(), N, C, HW,
                bn_ab.data_ptr() if bn_ab is not None else None, int(act), maxval.contiguous().data_ptr(),
                prep.data_ptr() if prep is not None else None, float(mbits), int(n_bits), int(sign_bits), _stream(x))
        check(rc, "fp8q_affine_act_quantize_ab_f32")
        return y
    ptrs, keep = _bn_ptrs(bn, C, x.device)
    with _on_device(x):
        rc = lib().fp8q_affine_act_quantize_f32(
            x.data_ptr(), residual.data_ptr() if residual is not None else None, y.data_ptr(), N, C, HW,
            ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(act), maxval.contiguous().data_ptr(), float(mbits),
            int(n_bits), int(sign_bits), _stream(x))
    check(rc, "fp8q_affine_act_quantize_f32")
    return y


def _affine_args(x, bn_ab, residual, out):
    """(x, residual, y, N, C, HW, alpha_beta pointer) of the epilogues that take the folded BN vector (affine_act, the INT fused epilogue)"""
    _require(x, "x")
    x = x.contiguous()
    N, C, HW = _nchw(x)
    if residual is not None:
        _require(residual, "residual", like=x)
        residual = residual.contiguous()
        if residual.shape != x.shape:
            raise Fp8qError("residual must have x's shape")
    if bn_ab is not None:
        _require(bn_ab, "bn_ab", like=x)
        if bn_ab.numel() != 2 * C or not bn_ab.is_contiguous():
            raise Fp8qError("bn_ab must be a contiguous [C, 2] tensor (fp8q.ops.bn_fold)")
    return x, residual, _out(out, x), N, C, HW, bn_ab.data_ptr() if bn_ab is not None else None


def affine_act(x, bn_ab=None, residual=None, act=0, out=None):
    """act(bn(x) + residual) without a quantizer (fp8q_affine_act_f32): what an MSE estimator behind a BN + activation searches
    on.  bn_ab: the folded [C, 2] vector of bn_fold(), or None."""
    x, residual, y, N, C, HW, pab = _affine_args(x, bn_ab, residual, out)
    with _on_device(x):
        rc = lib().fp8q_affine_act_f32(x.data_ptr(), residual.data_ptr() if residual is not None else None, y.data_ptr(), N, C, HW,
                                       pab, int(act), _stream(x))
    check(rc, "fp8q_affine_act_f32")
    return y


AFFINE_KERNELS = ("staged_nt", "small", "staged1", "staged4")      # FP8Q_AFFINE_* (include/fp8q.h)


def affine_act_route(N, C, HW, has_bn):
    """The kernel affine_act_quantize / affine_act reach for an [N, C, HW] tensor with or without a batch norm
    (fp8q_affine_act_route, include/fp8q.h), as a dict: kernel ("staged_nt" k_affine_act<true, 4>, "small" k_affine_act_small,
    "staged1" k_affine_act<false, 1>, "staged4" k_affine_act<false, 4>; None when nothing is launched), direct (the staged
    kernel keeps the BN constants of a piece's two planes in registers, not in LDS), cpp, launches, grid_x, grid_y (of the
    first launch).  Host arithmetic only: needs no GPU.  Raises Fp8qError as affine_act_quantize would for the shape."""
    import ctypes
    from ._lib import AffineRouteInfo
    info = AffineRouteInfo()
    check(lib().fp8q_affine_act_route(int(N), int(C), int(HW), int(bool(has_bn)), ctypes.byref(info)), "fp8q_affine_act_route")
    return {"kernel": AFFINE_KERNELS[info.kernel] if info.kernel >= 0 else None, "direct": bool(info.direct),
            "cpp": int(info.cpp), "launches": int(info.launches), "grid_x": int(info.grid_x), "grid_y": int(info.grid_y)}


def int_affine_act_quantize(x, delta, zero_float, signed_flag, n_bits, symmetric, eps, bn_ab=None, residual=None, act=0,
                            out=None):
    """N2 for the uniform quantizers: int_quantize(affine_act(x, bn_ab, residual, act)) in ONE pass
    (fp8q_int_affine_act_quantize_f32), bit for bit that composition.  Per-tensor ranges only: delta (and zero_float,
    asymmetric) of one element, signed_flag the symmetric quantizer's device byte; bn_ab: the folded [C, 2] vector of
    bn_fold() or None; act: 0 none, 1 ReLU, 2 ReLU6.  `out` may be x or residual."""
    x, residual, y, N, C, HW, pab = _affine_args(x, bn_ab, residual, out)
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, 1)      # per tensor: one element each
    with _on_device(x):
        rc = lib().fp8q_int_affine_act_quantize_f32(x.data_ptr(), residual.data_ptr() if residual is not None else None,
                                                    y.data_ptr(), N, C, HW, pab, int(act), pd, pz, ps, int(n_bits),
                                                    int(bool(symmetric)), float(eps), _stream(x))
    check(rc, "fp8q_int_affine_act_quantize_f32")
    return y


def int_affine_act_range_quantize(x, x_min, x_max, n_bits, symmetric, eps, delta=None, zero_float=None, signed_flag=None,
                                  bn_ab=None, residual=None, act=0, out=None):
    """int_set_range(x_min, x_max) and int_affine_act_quantize in ONE launch (fp8q_int_affine_act_range_quantize_f32): the
    range-estimating forward behind a BN / residual / activation.  x_min, x_max: one element each.  Returns
    (y, delta, zero_float, signed_flag) like int_range_quantize; buffers passed in are written in place."""
    x, residual, y, N, C, HW, pab = _affine_args(x, bn_ab, residual, out)
    _require(x_min, "x_min", like=x)
    _require(x_max, "x_max", like=x)
    x_min, x_max = x_min.detach().contiguous(), x_max.detach().contiguous()
    if x_min.numel() != 1 or x_max.numel() != 1:
        raise Fp8qError("the fused epilogue quantizes per tensor: x_min and x_max must have one element")
    n, delta, zero_float, signed_flag = _int_range_out(x_min, delta, zero_float, signed_flag, symmetric)
    pd, pz, ps = _int_ptrs(x, delta, zero_float, signed_flag, symmetric, 1)
    if N == 0:
        return (y,) + int_set_range(x_min, x_max, n_bits, symmetric, eps, delta, zero_float, signed_flag)
    with _on_device(x):
        rc = lib().fp8q_int_affine_act_range_quantize_f32(
            x.data_ptr(), residual.data_ptr() if residual is not None else None, y.data_ptr(), N, C, HW, pab, int(act),
            x_min.data_ptr(), x_max.data_ptr(), pd, pz, ps, int(n_bits), int(bool(symmetric)), float(eps), _stream(x))
    check(rc, "fp8q_int_affine_act_range_quantize_f32")
    return y, delta, zero_float, signed_flag


def affine_act_minmax(x, cur_min=None, cur_max=None, mode=FOLD_CURRENT, momentum=0.9, bn=None, residual=None,
                      act=0, packed=None):
    """N2: per-tensor min/max of act(bn(x) + residual), folded into the running estimate.
    packed: optional [1, 4] buffer for the range all-reduce (see minmax).
    Returns (cur_min, cur_max, maxval) as [1] tensors."""
    _require(x, "x")
    x = x.contiguous()
    N, C, HW = _nchw(x)
    if residual is not None:
        _require(residual, "residual", like=x)
        residual = residual.contiguous()
        if residual.shape != x.shape:
            raise Fp8qError("residual must have x's shape")
    ptrs, keep = _bn_ptrs(bn, C, x.device)
    first = cur_min is None or cur_max is None
    if first:
        cur_min = torch.empty(1, dtype=torch.float32, device=x.device)
        cur_max = torch.empty(1, dtype=torch.float32, device=x.device)
    else:
        for t in (cur_min, cur_max):
            _require(t, "running estimate", like=x)
            if t.numel() != 1 or not t.is_contiguous():
                raise Fp8qError("running estimate has the wrong shape")
    mv = torch.empty(1, dtype=torch.float32, device=x.device)
    L = lib()
    ws = _workspace(x.device, L.fp8q_affine_act_minmax_workspace_bytes(N, C, HW), zeroed=True)
    with _on_device(x):
        if packed is None:
            rc = L.fp8q_affine_act_minmax_f32(
                x.data_ptr(), residual.data_ptr() if residual is not None else None, N, C, HW, ptrs[0], ptrs[1],
                ptrs[2], ptrs[3], int(act), cur_min.data_ptr(), cur_max.data_ptr(), mv.data_ptr(), int(mode),
                float(momentum), int(first), ws.data_ptr(), ws.numel(), _stream(x))
        else:
            _check_packed(packed, 1)
            _require(packed, "packed", like=x)
            rc = L.fp8q_affine_act_minmax_packed_f32(
                x.data_ptr(), residual.data_ptr() if residual is not None else None, N, C, HW, ptrs[0], ptrs[1],
                ptrs[2], ptrs[3], int(act), cur_min.data_ptr(), cur_max.data_ptr(), mv.data_ptr(), packed.data_ptr(),
                int(mode), float(momentum), int(first), ws.data_ptr(), ws.numel(), _stream(x))
    check(rc, "fp8q_affine_act_minmax_f32")
    return cur_min, cur_max, mv
