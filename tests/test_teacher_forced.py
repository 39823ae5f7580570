"""Teacher-forced per-quantizer parity with the reference on ResNet-18 (config 3) and MobileNetV2 (config 4, with and
without the mantissa-width search), fixture G13 (tests/golden/make_golden.py: make_g13).

test_models.py compares whole calibrated networks, where one rounding difference cascades through every later layer,
so its assertions are bounds.  Here every quantizer is fed the reference's OWN input -- each hijacked layer's
run_forward output and both addends of each residual add are substituted by the reference's -- so nothing cascades and
every call is held to the same criteria (_check):
  min/max estimators  xmin, xmax, maxval bit-equal (NaN pattern included);
  MSE                 search grid bit-equal, per-tensor tables within rtol 1e-4 of the reference and 1e-5 of the oracle,
                      mantissa width and maxval equal -- unless the reference's own table value at the chosen
                      (width, candidate) is within 1e-6 of its minimum (a near tie; needs a stored table);
  outputs             parity.assert_parity against the reference's output where (maxval, mbits) agree, bit-equal to the
                      oracle at the chosen (maxval, mbits) where a near tie decided otherwise.
"""
import copy
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

import oracle
from parity import assert_parity, elem_step
from test_models import _managers, _warm_bn

CONFIGS = {"g13_r18": ("r18", 2, "current_minmax", "allminmax", False),
           "g13_mbv2": ("mbv2", 3, "MSE", "MSE", False),
           "g13_mbv2m": ("mbv2", 3, "MSE", "MSE", True)}
N_MGR = {"r18": 50, "mbv2": 123}
N_CALLS = {"r18": 50, "mbv2": 116}          # MobileNetV2: the blocks without a skip never run their own quantizer
SIZE = 32
NEAR_TIE = 1e-6


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _ulp_key(a):
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, np.int64(-2147483648) - i, i)


def _from_ulp_key(k):
    return np.where(k >= 0, k, np.int64(-2147483648) - k).astype(np.int32).view(np.float32)


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


class G13:
    """One configuration of the fixture; records which arrays the caller consumed."""

    def __init__(self, golden_dir, fname):
        raw = np.load(os.path.join(golden_dir, f"{fname}.npz"))
        self.g = {}
        for key in raw.files:                      # make_golden.py:_g13_pack -> c<k>_<what>
            if key.startswith("pack_") and key.endswith("_index"):
                data = raw[key[:-len("_index")]]
                for k, off, shape in json.loads(str(raw[key])):
                    self.g[f"c{k}_{key[5:-6]}"] = data[off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape)
            elif not key.startswith("pack_"):
                self.g[key] = raw[key]
        self.sub = np.load(os.path.join(golden_dir, f"{fname}_sub.npz"))
        self.calls = json.loads(str(self.g["calls"]))
        self.used = {"calls", "managers", "calib"}
        self.used_sub = set()

    def arr(self, key):
        self.used.add(key)
        return self.g[key]

    def run(self, layer):
        self.used_sub.add(f"run_{layer}")
        return self.sub[f"run_{layer}"]

    def rebuild(self, key, base):
        """the reference's tensor from the oracle's recomputation `base` + the stored sparse ULP diff; checked by hash"""
        y = np.ascontiguousarray(base, np.float32).reshape(-1).copy()
        idx = np.cumsum(self.arr(f"{key}_idx_delta").astype(np.int64))
        y[idx] = _from_ulp_key(_ulp_key(y[idx]) + self.arr(f"{key}_ulp_delta").astype(np.int64))
        y[self.arr(f"{key}_big_idx")] = self.arr(f"{key}_big_val")
        assert np.array_equal(_sha(y), self.arr(f"{key}_sha256")), f"{key}: rebuilt tensor does not match its hash"
        return y.reshape(np.shape(base))


def _qparams(M, w_est, a_est, incl):
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    return dict(method=QMethods.fp_quantizer.cls, weight_range_method=RangeEstimators[w_est].cls,
                act_range_method=RangeEstimators[a_est].cls, n_bits=8, n_bits_act=8, per_channel_weights=True,
                fp8_kwargs=dict(maxval=None, mantissa_bits=M, set_maxval=True, learn_maxval=False,
                                learn_mantissa_bits=False, mse_include_mantissa_bits=incl, allow_unsigned=False))


def _build(fname, golden_dir):
    """this repo's quantized model of the configuration, built as make_g13 builds the reference's, with the reference's
    BN running statistics (warm_bn's CPU reductions need not agree bit for bit on another machine)"""
    from quantization.layers import BNFusedHijacker
    q = _build_net(fname)
    g = np.load(os.path.join(golden_dir, f"{fname}.npz"))
    for n, m in q.named_modules():
        if isinstance(m, BNFusedHijacker):
            mean, var, _ = torch.from_numpy(g[f"bn_{n}"])
            m.running_mean.copy_(mean)
            m.running_var.copy_(var)
    return q


def _build_net(fname):
    model, M, w_est, a_est, incl = CONFIGS[fname]
    torch.manual_seed(0)
    if model == "r18":
        from models.resnet import resnet18
        from models.resnet_quantized import QuantizedResNet
        return QuantizedResNet(_warm_bn(resnet18()), input_size=(1, 3, SIZE, SIZE),
                               **_qparams(M, w_est, a_est, incl)).eval()
    from models.mobilenet_v2 import MobileNetV2
    from models.mobilenet_v2_quantized import QuantizedMobileNetV2
    warm = _warm_bn(MobileNetV2(input_size=64))
    fp = MobileNetV2(input_size=SIZE).eval()        # AvgPool2d is sized at construction
    fp.load_state_dict(warm.state_dict())
    return QuantizedMobileNetV2(fp, input_size=(1, 3, SIZE, SIZE), **_qparams(M, w_est, a_est, incl)).eval()


def _mbit_list(fname):
    _, M, _, _, incl = CONFIGS[fname]
    return [float(m) for m in range(1, 7)] if incl else [float(M)]


def _np(t):
    return t.detach().float().cpu().numpy()


def _ref_grid(x):
    """range_estimators.py:296-305: per channel torch.linspace(0.1 * mx.item(), 1.2 * mx.item(), 111)"""
    mn, mx = oracle.c_minmax(x, True)
    mxs = oracle.c_absmax(mn, mx)
    return torch.stack([torch.linspace(0.1 * float(v), 1.2 * float(v), 111) for v in mxs], 1).numpy()


def _call_input(g, call, mods):
    """(the reference's quantizer input, (pre, bn, residual) for an activation call or None)"""
    k = call["k"]
    if call["kind"] == "weight":
        x = _np(mods[call["name"].rsplit(".", 1)[0]].weight)
        assert np.array_equal(_sha(x), g.arr(f"c{k}_x_sha256")), f"{call['name']}: not the reference's weight"
        return x, None
    o = call["owner"]
    if call["residual"]:
        pre, res, bn = g.arr(f"res_{o}_branch"), g.arr(f"res_{o}_skip"), None
    else:
        pre, res = g.run(o), None
        if call["bn"]:               # 1 / sqrt(var + eps) as make_g13 formed it (torch's vectorised CPU code varies by machine)
            m = mods[o]
            bn = (_np(m.running_mean), g.arr(f"bn_{o}")[2], _np(m.gamma), _np(m.beta))
        else:
            bn = None
    return g.rebuild(f"c{k}_x", oracle.c_affine_act(pre, bn, res, call["act"])), (pre, bn, res)


def _ref_state(g, call, x, fname):
    k = call["k"]
    r = dict(maxval=g.arr(f"c{k}_maxval"), mbits=call["mbits"], sign_bits=call["sign_bits"], table=None)
    r["y"] = g.rebuild(f"c{k}_y", oracle.c_quantize(x, r["maxval"], r["mbits"], 8, r["sign_bits"]))
    if call["est"] == "FP_MSE_Estimator":
        if not call["per_channel"]:
            r["grid"], r["mses"] = g.arr(f"c{k}_grid"), g.arr(f"c{k}_mses")
            r["table"] = {0: r["mses"][:, :, 0]}
        else:
            grid = _ref_grid(x)
            assert np.array_equal(_sha(grid), g.arr(f"c{k}_grid_sha256")), call["name"]
            r["grid"] = grid
            arg, best_m = g.arr(f"c{k}_argmin").astype(np.int64), g.arr(f"c{k}_best_m").astype(np.int64)
            assert _bits_equal(grid[arg, np.arange(grid.shape[1])], r["maxval"]), call["name"]
            vote = _mbit_list(fname).index(r["mbits"])
            assert np.bincount(best_m, minlength=len(_mbit_list(fname))).argmax() == vote, call["name"]   # torch.mode
            r["table"] = dict(zip(g.arr(f"c{k}_tie_ch").tolist(), g.arr(f"c{k}_tie_rows")))
    else:
        r["xmin"], r["xmax"] = g.arr(f"c{k}_xmin"), g.arr(f"c{k}_xmax")
    return r


def _decoded(golden_dir, fname, mods):
    """[(call, x, pre_info, ref)] in calibration order; every stored array consumed"""
    g = G13(golden_dir, fname)
    out = []
    for call in g.calls:
        x, pre = _call_input(g, call, mods)
        out.append((call, x, pre, _ref_state(g, call, x, fname)))
    assert g.used == set(g.g), sorted(set(g.g) - g.used)[:8]
    assert g.used_sub == set(g.sub.files), sorted(set(g.sub.files) - g.used_sub)[:8]
    return g, out


def _state(mgr, y):
    q, est = mgr.quantizer, mgr.range_estimator
    s = dict(maxval=_np(q.maxval).reshape(-1), mbits=float(q.mantissa_bits), sign_bits=int(q.sign_bits), y=_np(y))
    if type(est).__name__ == "FP_MSE_Estimator":
        s["grid"], s["mses"] = _np(est.search_grid), _np(est.mses)
    else:
        s["xmin"], s["xmax"] = _np(est.current_xmin).reshape(-1), _np(est.current_xmax).reshape(-1)
    return s


def _check(fname, call, x, ref, got, stats):
    """the per-call criteria of the module docstring; counts near-tie exemptions and the largest ULP difference"""
    what = f"{fname} {call['name']}"
    mv_ref, mv = np.asarray(ref["maxval"], np.float32).reshape(-1), got["maxval"]
    assert got["sign_bits"] == ref["sign_bits"], what
    if call["est"] != "FP_MSE_Estimator":
        assert _bits_equal(got["xmin"], ref["xmin"]) and _bits_equal(got["xmax"], ref["xmax"]), what
        assert _bits_equal(mv, mv_ref) and got["mbits"] == ref["mbits"], what
        same = np.ones(mv_ref.size, bool)
    else:
        grid = ref["grid"]
        if call["per_channel"]:
            assert np.array_equal(_sha(got["grid"]), _sha(grid)), f"{what}: search grid"
        else:
            assert _bits_equal(got["grid"], grid), f"{what}: search grid"
            np.testing.assert_allclose(got["mses"], ref["mses"], rtol=1e-4, atol=0, err_msg=what)
            orc = oracle.c_mse_grid(x, False, grid, _mbit_list(fname), 8, ref["sign_bits"])
            np.testing.assert_allclose(got["mses"], orc, rtol=1e-5, atol=0, err_msg=what)
        assert mv.size == mv_ref.size, what
        same = mv.view(np.int32) == mv_ref.view(np.int32)
        if got["mbits"] != ref["mbits"]:
            assert not call["per_channel"], f"{what}: voted width {got['mbits']} != {ref['mbits']}"
            same[:] = False
        for c in np.flatnonzero(~same):          # the near-tie rule
            table = ref["table"].get(int(c))
            assert table is not None, f"{what}: channel {c}: maxval {mv[c]!r} != {mv_ref[c]!r}, not a near tie"
            i = np.flatnonzero(grid[:, c].view(np.int32) == mv[c:c + 1].view(np.int32))
            assert i.size, f"{what}: channel {c}: maxval {mv[c]!r} is not a grid value"
            val = table[_mbit_list(fname).index(got["mbits"]), i[0]]
            assert val <= (1 + NEAR_TIE) * table.min(), f"{what}: channel {c}: {val} vs min {table.min()}"
            stats["exempt"] += 1
    y, y_ref = got["y"], ref["y"]
    assert y.shape == y_ref.shape, what
    rows = same if mv_ref.size > 1 else np.full(y.shape[0] if call["per_channel"] else 1, bool(same[0]))
    y2, yr2, x2 = (a.reshape(rows.size, -1) for a in (y, y_ref, x))
    if rows.any():
        mvs = mv_ref[rows] if mv_ref.size > 1 else mv_ref
        r = assert_parity(y2[rows], yr2[rows], elem_step(x2[rows], mvs, ref["mbits"], 8, ref["sign_bits"]), what=what)
        stats["max_ulp"] = max(stats["max_ulp"], r["max_ulp_nonflip"])
        stats["flips"] += r["n_flips"]
    if not rows.all():
        mvs = mv[~rows] if mv.size > 1 else mv
        assert _bits_equal(y2[~rows], oracle.c_quantize(x2[~rows], mvs, got["mbits"], 8, got["sign_bits"])), what


def _check_own_input(fname, call, x, got, stats):
    """an activation call whose input is not the reference's after all (FP8Q_FUSE_EPILOGUE=0: torch's GPU batch_norm is
    not the CPU one bit for bit): the same criteria with the C oracle on that input as the reference"""
    what = f"{fname} {call['name']} (own input)"
    assert call["kind"] == "act" and not call["per_channel"], what
    stats["own_input"] += 1
    mv = got["maxval"]
    if call["est"] != "FP_MSE_Estimator":
        mn, mx = oracle.c_minmax(x, False)
        assert _bits_equal(got["xmin"], mn) and _bits_equal(got["xmax"], mx), what
        assert _bits_equal(mv, oracle.c_absmax(mn, mx)), what
    else:
        grid = _ref_grid(x.reshape(1, -1))
        assert _bits_equal(got["grid"], grid), f"{what}: search grid"
        orc = oracle.c_mse_grid(x, False, grid, _mbit_list(fname), 8, call["sign_bits"])
        np.testing.assert_allclose(got["mses"], orc, rtol=1e-5, atol=0, err_msg=what)
        i = np.flatnonzero(grid[:, 0].view(np.int32) == mv[:1].view(np.int32))
        assert i.size, f"{what}: maxval {mv[0]!r} is not a grid value"
        val = orc[_mbit_list(fname).index(got["mbits"]), i[0], 0]
        assert val <= (1 + NEAR_TIE) * orc.min(), f"{what}: {val} vs min {orc.min()}"
        stats["exempt"] += int(val != orc.min())
    assert _bits_equal(got["y"], oracle.c_quantize(x, mv, got["mbits"], 8, got["sign_bits"])), what


def _new_stats():
    return dict(exempt=0, max_ulp=0, flips=0, own_input=0)


def _report(tag, fname, stats):
    print(f"\n{tag} {fname}: {stats['exempt']} near-tie exemptions, largest ULP difference {stats['max_ulp']}, "
          f"{stats['flips']} grid-step flips, {stats['own_input']} calls checked on their own input")


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", list(CONFIGS))
def test_g13_decodes(golden_dir, fname):
    """Every stored tensor rebuilds to its hash, every stored array is consumed, one call per manager the reference ran."""
    model = CONFIGS[fname][0]
    q = _build(fname, golden_dir)
    mods = dict(q.named_modules())
    g, dec = _decoded(golden_dir, fname, mods)
    names = [n for n, _ in _managers(q)]
    assert len(names) == N_MGR[model] and names == [str(n) for n in g.g["managers"]]
    called = [c["name"] for c, *_ in dec]
    assert len(called) == N_CALLS[model] and len(set(called)) == len(called)
    assert set(called) <= set(names)
    n_w = sum(c["kind"] == "weight" for c, *_ in dec)
    assert n_w == sum(n.endswith("weight_quantizer") for n in names)
    assert g.g["calib"].shape == (2, 3, SIZE, SIZE)
    torch.manual_seed(13)
    assert np.array_equal(g.g["calib"], torch.randn(2, 3, SIZE, SIZE).numpy())


@pytest.mark.parametrize("fname", list(CONFIGS))
def test_per_call_oracle_backend(golden_dir, fname):
    """Each of this repo's managers, fresh, fed the reference's input on the CPU oracle backend (the host logic and the
    oracle's arithmetic, without MIOpen / rocBLAS between the calls)."""
    import oracle_ops
    q = _build(fname, golden_dir)
    mods, mgrs = dict(q.named_modules()), dict(_managers(q))
    _, dec = _decoded(golden_dir, fname, mods)
    stats = _new_stats()
    with oracle_ops.patched(), torch.no_grad():
        for call, x, _, ref in dec:
            mgr = mgrs[call["name"]]
            y = mgr(torch.from_numpy(x.copy()))
            _check(fname, call, x, ref, _state(mgr, y), stats)
    _report("oracle backend", fname, stats)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("fname", list(CONFIGS))
def test_per_call_hip(golden_dir, fname):
    """Each manager through QuantizationManager.forward on the reference's input; where the model fuses the producer's
    epilogue, a second fresh manager through forward_fused(pre, bn, residual, act) as well.  Both meet the criteria; their
    outputs are bit-identical wherever their inputs are (the fused path forms act(bn(pre) + residual) itself)."""
    qa, qb = _build(fname, golden_dir).cuda(), _build(fname, golden_dir).cuda()
    mods_cpu = dict(_build(fname, golden_dir).named_modules())
    mgr_a, mgr_b, mods_b = dict(_managers(qa)), dict(_managers(qb)), dict(qb.named_modules())
    _, dec = _decoded(golden_dir, fname, mods_cpu)
    stats, n_fused = _new_stats(), 0
    with torch.no_grad():
        for call, x, pre, ref in dec:
            mgr = mgr_a[call["name"]]
            y = mgr(_cuda(x))
            sa = _state(mgr, y)
            _check(fname, call, x, ref, sa, stats)
            if pre is None:
                continue
            p, _, res = pre
            owner, mb = mods_b[call["owner"]], mgr_b[call["name"]]
            pc = _cuda(p)
            if not mb.can_fuse(pc):
                continue
            bn = owner._bn_vectors() if call["bn"] else None
            ab = owner._bn_folded() if call["bn"] else None
            yb = mb.forward_fused(pc, bn=bn, residual=_cuda(res), act=call["act"], bn_ab=ab)
            xb = oracle.c_affine_act(p, None if bn is None else tuple(_np(t) for t in bn), res, call["act"])
            sb = _state(mb, yb)
            _check(fname, call, xb, ref, sb, stats)
            n_fused += 1
            assert _bits_equal(sa["maxval"], sb["maxval"]) and sa["mbits"] == sb["mbits"], call["name"]
            same_in = xb.reshape(-1).view(np.int32) == x.reshape(-1).view(np.int32)
            assert np.array_equal(sa["y"].reshape(-1)[same_in].view(np.int32), sb["y"].reshape(-1)[same_in].view(np.int32)), \
                f"{call['name']}: fused and unfused outputs differ"
    assert n_fused > 0
    _report(f"HIP per call ({n_fused} fused)", fname, stats)


class _Teacher:
    """Substitutes the reference's tensors into this repo's model on the GPU: every hijacked layer's run_forward returns
    the reference's output (after checking the quantized weight it was handed), every residual add gets the reference's
    addends; records what every manager returned, through forward or forward_fused (which bypasses module hooks)."""

    def __init__(self, q, g):
        from quantization.layers import QuantizationHijacker
        from quantization.quantization_manager import QuantizationManager
        from models.mobilenet_v2_quantized import QuantizedInvertedResidual
        from models.resnet_quantized import QuantizedBlock
        self.q, self.weights, self.outs, self.handles, self.patched = q, {}, {}, [], []
        self.fused_depth = 0
        names = {id(m): n for n, m in _managers(q)}
        for n, m in q.named_modules():
            if isinstance(m, QuantizationHijacker):
                self._patch(m, "run_forward", self._run_forward(n, _cuda(g.run(n))))
            if isinstance(m, (QuantizedBlock, QuantizedInvertedResidual)) and getattr(m, "use_res_connect", True):
                branch, skip = _cuda(g.arr(f"res_{n}_branch")), _cuda(g.arr(f"res_{n}_skip"))
                main = m.features if isinstance(m, QuantizedBlock) else m.conv
                self.handles.append(main.register_forward_hook(lambda mod, a, y, t=branch: t.clone()))
                if getattr(m, "downsample", None) is not None:
                    self.handles.append(m.downsample.register_forward_hook(lambda mod, a, y, t=skip: t.clone()))
                else:
                    self.handles.append(m.register_forward_pre_hook(lambda mod, a, t=skip: (t.clone(),)))
            if isinstance(m, QuantizationManager) and id(m) in names:
                self.handles.append(m.register_forward_hook(self._mgr_hook(names[id(m)])))
                self._patch(m, "forward_fused", self._fused(names[id(m)], m.forward_fused))

    def _patch(self, m, attr, fn):
        m.__dict__[attr] = fn
        self.patched.append((m, attr))

    def _run_forward(self, name, t):
        def run_forward(x, weight, bias, offsets=None):
            self.weights.setdefault(name, []).append(weight.detach().clone())
            return t.clone()
        return run_forward

    def _mgr_hook(self, name):
        def hook(mod, args, y):
            if not self.fused_depth:
                self.outs.setdefault(name, []).append((args[0].detach().clone(), None, y.detach().clone()))
        return hook

    def _fused(self, name, orig):
        def forward_fused(x, bn=None, residual=None, act=0, bn_ab=None):
            self.fused_depth += 1
            try:
                y = orig(x, bn=bn, residual=residual, act=act, bn_ab=bn_ab)
            finally:
                self.fused_depth -= 1
            pre = (_np(x), None if bn is None else tuple(_np(t) for t in bn), None if residual is None else _np(residual), act)
            self.outs.setdefault(name, []).append((None, pre, y.detach().clone()))
            return y
        return forward_fused

    def forward(self, x):
        self.weights, self.outs = {}, {}
        with torch.no_grad():
            self.q(x)
        torch.cuda.synchronize()
        return self.weights, self.outs

    def remove(self):
        for h in self.handles:
            h.remove()
        for m, attr in self.patched:
            del m.__dict__[attr]
        self.handles, self.patched = [], []


def _in_loop_calibrate(golden_dir, fname, fuse="1"):
    """calibrate this repo's model (estimate state, one batch) on the GPU under teacher forcing; check every call"""
    q = _build(fname, golden_dir)
    mods_cpu = dict(_build(fname, golden_dir).named_modules())
    g, dec = _decoded(golden_dir, fname, mods_cpu)
    q = q.cuda()
    q.set_quant_state(True, True)
    teacher = _Teacher(q, g)
    calib = _cuda(g.g["calib"])
    weights, outs = teacher.forward(calib)
    mgrs = dict(_managers(q))
    assert sorted(outs) == sorted(c["name"] for c, *_ in dec), "managers called differ from the reference's"
    stats = _new_stats()
    for call, x_ref, _, ref in dec:
        rec = outs[call["name"]]
        assert len(rec) == 1, f"{call['name']} called {len(rec)} times"
        x_in, pre, y = rec[0]
        x = _np(x_in) if pre is None else oracle.c_affine_act(*pre)
        if _bits_equal(x, x_ref):
            _check(fname, call, x, ref, _state(mgrs[call["name"]], y), stats)
        else:
            # only torch's own GPU batch_norm (the unfused epilogue) may move a quantizer's input off the reference's
            assert fuse == "0" and call["bn"], f"{call['name']}: the quantizer did not see the reference's input"
            _check_own_input(fname, call, x, _state(mgrs[call["name"]], y), stats)
        if call["kind"] == "weight":
            w = weights[call["name"].rsplit(".", 1)[0]]
            assert len(w) == 1 and torch.equal(w[0], y), f"{call['name']}: run_forward got another weight"
    return q, teacher, calib, weights, outs, stats


def _fixed_pass_matches(teacher, calib, weights, outs, what):
    """after fix_ranges(): the substituted forward gives every quantizer's calibration-pass output again, bit for bit"""
    w2, o2 = teacher.forward(calib)
    assert sorted(w2) == sorted(weights)
    for n, ws in w2.items():
        assert len(ws) == 1 and torch.equal(ws[0].view(torch.int32), weights[n][0].view(torch.int32)), f"{what}: weight {n}"
    for n, rec in outs.items():
        if n.endswith("weight_quantizer"):
            continue                   # fixed weights come from the layer's cache (the plan), checked above
        assert len(o2.get(n, ())) == 1, f"{what}: {n}"
        assert torch.equal(o2[n][0][2].view(torch.int32), rec[0][2].view(torch.int32)), f"{what}: output of {n}"


@pytest.mark.gpu
@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("fname", list(CONFIGS))
def test_in_loop_hip(golden_dir, fname, fuse, monkeypatch):
    """The repo's real model on the GPU, every layer's output and residual addend replaced by the reference's: the
    lookahead weight stream, the fused epilogue (FP8Q_FUSE_EPILOGUE=1), the one-call MSE path, the device-side vote and
    fix_ranges() collecting it."""
    monkeypatch.setenv("FP8Q_FUSE_EPILOGUE", fuse)
    q, teacher, calib, weights, outs, stats = _in_loop_calibrate(golden_dir, fname, fuse)
    q.fix_ranges()
    _fixed_pass_matches(teacher, calib, weights, outs, fname)
    teacher.remove()
    _report(f"HIP in the loop (fused epilogue {fuse})", fname, stats)


@pytest.mark.gpu
def test_copy_after_mse_calibration(golden_dir):
    """copy.deepcopy and torch.save / torch.load of a model after a GPU MSE calibration (its estimators hold native
    calibration state, its layers what the lookahead weight stream left); the copy fixes the same ranges and can go on
    calibrating."""
    fname = "g13_mbv2"
    q, teacher, calib, weights, outs, _ = _in_loop_calibrate(golden_dir, fname)
    teacher.remove()
    dup = copy.deepcopy(q)
    buf = io.BytesIO()
    torch.save(q, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    g = G13(golden_dir, fname)
    for m in (q, dup):
        m.fix_ranges()
        t = _Teacher(m, g)
        _fixed_pass_matches(t, calib, weights, outs, "copy" if m is dup else "original")
        t.remove()
    torch.manual_seed(14)
    with torch.no_grad():
        y = loaded(torch.randn(2, 3, SIZE, SIZE, device="cuda"))      # a second calibration batch
    loaded.fix_ranges()
    assert torch.isfinite(y).all() and y.shape == (2, 1000)
