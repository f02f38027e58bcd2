"""The two Part 4 chains (csrc/p4mlp.hip) restated in torch, as functions of the hash FEATURES handed to them -- for the tests.

A helper module, not a test (family: tests/hashgrid_reference.py, tests/frontend_reference.py).  The field is cut at the hash
features, so no hash cell is ever crossed: what is left is two small networks whose arithmetic can be matched rounding by rounding.

  deformation chain   tcode = [Fourier_10(t) | 1]; tm = sigmoid(T2 relu(T1 tcode) + b_T2); df = sum_k w_k(t) feat_k;
                      raw = D3 relu(D2 relu(D1 [df | tm])); dx = raw * scale; x_c = x + dx
  canonical chain     InstantNeRFDecoder on [hash 32 | Fourier_10(t) 21] and Fourier_4(dir): tests/test_instant_shapes_layout.py::chain64
                      with this file's rounding points (the kernel bodies are instant_chain_body.h's)

``rounded=False``: plain arithmetic in ``dtype`` (float64: the restatement of reference src/core.py:282-352 behind the hash grids).
``rounded=True``: rounds where the kernels round and nowhere else; sums in ``dtype`` (float64 for the reference, float32 for the
yardstick's other side).  Backward = autograd of ``dtype`` with straight-through rounding (tests/test_gpu_parity.py::_Q's style).

Rounding points (file:line of project-nerf_amd/csrc at the time of writing)
  forward, fp16
    p4mlp.hip:102       weights of T1 (with b_T1 as column 21), T2, D1, D2, D3, S1, S2, C1, C2, C3 -> fp16 fragments; b_T2 stays fp32 (:104)
    p4mlp.hip:141       time code (with the constant-1 column, :118) and direction code -> fp16 operands (cast_values)
    resident_chain.h:132, mlp_chain.h acc_to_operand16   relu(T1), relu(D1), relu(D2), relu(S1), relu(C1), relu(C2) -> fp16
    p4mlp.hip:214       the gate sigmoid(acc + b_T2) -> fp16
    p4mlp.hip:230-231   the blend w0 f0 + w1 f1 + w2 f2 (fp32, of fp16 features) -> fp16
    p4mlp.hip:146, :433 the hash features arrive as fp16 images
    instant_chain_body.h:44   h = S2's 16 outputs -> fp16 operand of C1; sigma takes the fp32 acc[0] (:43, :47)
    not rounded: dx = acc * scale (p4mlp.hip:253), rgb, sigma (resident_chain.h:148-155)
  backward, bf16
    p4mlp.hip:102       weights of D3t, D2t, D1tT, D1tH, T2t, C3t, C2t, C1t, S2t, S1t -> bf16 fragments
    p4mlp.hip:362, :366 fp32 d_dx * scale -> bf16 (small_operand, resident_chain.h:110)
    resident_chain.h:163-165, :110   d_rgb r (1 - r) -> bf16
    resident_chain.h:140-141   masked pre-activation gradients of D2, D1, T1, C2, C1, S1 -> bf16 (operand and image); the mask is the
                               bit acc > 0 of the forward's fp32 accumulator (resident_chain.h:118)
    p4mlp.hip:379-383   d(tm) s (1 - s) with s the STASHED bf16 gate -> bf16
    instant_chain_body.h:164-165   d(h) = C1t's tile + softplus' d_sigma on row 0 -> bf16
    not rounded: d_feat (p4mlp.hip:393, instant_chain_body.h:132), g_scale = sum d_dx raw with the fp32 raw (p4mlp.hip:363)
  training images, bf16 (the weight gradients' second operand, mlp_wgrad.hip)
    p4mlp.hip:141, :236-239   time code, constant 1, blend (rounded from the fp32 value, not from the fp16 operand)
    resident_chain.h:99-101   relu(T1), gate, relu(D1), relu(D2), relu(S1), h, relu(C1), relu(C2): rounded again from the fp32 acc
    p4mlp.hip:480       canonical hash features: bf16 of the fp16 image
    p4mlp.hip:141, :490 direction code

``MUTATIONS``: deliberately wrong references for sensitivity checks.
"""
import math

import numpy as np
import torch

from oracle import nerf_oracle as O

T1W, T1B, T2W, T2B, D1, D2, D3, S1, S2, C1, C2, C3, SCALE, N_PARAMS = (0, 1344, 1408, 5504, 5568, 11712, 15808, 16832, 20928, 21952, 25024,
                                                                          29120, 30144, 30145)
# (name, offset, stored shape, live shape) of the 13 parameter blocks: the layout at the top of p4mlp.hip
BLOCKS = (("T1W", T1W, (64, 21), (64, 21)), ("T1b", T1B, (64,), (64,)), ("T2W", T2W, (64, 64), (64, 64)), ("T2b", T2B, (64,), (64,)),
          ("D1", D1, (64, 96), (64, 88)), ("D2", D2, (64, 64), (64, 64)), ("D3", D3, (16, 64), (3, 64)),
          ("S1", S1, (64, 64), (64, 53)), ("S2", S2, (16, 64), (16, 64)),
          ("C1", C1, (64, 48), (64, 43)), ("C2", C2, (64, 64), (64, 64)), ("C3", C3, (16, 64), (3, 64)), ("scale", SCALE, (1,), (1,)))
DEFORM_BLOCKS = ("T1W", "T1b", "T2W", "T2b", "D1", "D2", "D3", "scale")
CANON_BLOCKS = ("S1", "S2", "C1", "C2", "C3")
# input blocks of the three layers that concatenate: (block, name, first column, end column)
INPUT_BLOCKS = (("D1", "D1[hash]", 0, 24), ("D1", "D1[tm]", 24, 88), ("S1", "S1[hash]", 0, 32), ("S1", "S1[tcode]", 32, 53),
                ("C1", "C1[h16]", 0, 16), ("C1", "C1[dir]", 16, 43))
MUTATIONS = (None, "swap_blend_weights", "drop_gate_derivative", "shift_time_band")
SHIFTED_TIME_COLUMN = 7          # sin(2^3 pi t): "shift_time_band" evaluates it at band 4

LEVELS_D, LEVELS_C, BOUND = (12, 10, 16, 1.5), (16, 11, 16, 1.5), 1.5        # PART4_CFG's level tables (tests/test_gpu_part4.py)
SWEEP = (1, 31, 32, 33, 127, 128, 129, 257, 1025)
N_POOL = 1025

# floors of the GPU bounds and the caps no bound may exceed (what they are: tests/test_part4_reference.py)
FLOOR_BF16, FLOOR_FP16, FLOOR_FP32 = 2.0 ** -9, 2.0 ** -11, 1e-6
CAP_FORWARD, CAP_GRAD = 2e-3, 2e-2


def _rnd(x, fmt):
    """x -> fmt -> x.dtype, through fp32: the chains' values are fp32 before they are rounded"""
    return x.detach().float().to(fmt).to(x.dtype)


def _st(x, fmt, rounded):
    """straight-through rounding: the value of fmt, the gradient of x"""
    return x + (_rnd(x, fmt) - x.detach()) if rounded else x


def _img(x, rounded):
    """the bf16 training image of an fp32 value (no gradient: autograd reaches the weights through _Lin)"""
    return _rnd(x, torch.bfloat16) if rounded else x.detach()


ORDERS = (16, 8, 32, 64)        # the float32 side's k-block (16: the MFMA's); every block length of _mm scales with it
_ORDER = [16]


def _mm(a, b, block):
    """a @ b^T for a [m,k], b [n,k].  float64: the plain product.  float32 (the yardstick's other side): a summation order DEFINED
    here, so that the yardstick does not depend on the machine's BLAS -- blocks of ``block`` terms summed exactly (float64 of exact
    fp32 products), each block rounded to fp32 and added to the fp32 running sum in order, the shape of an MFMA accumulating k-blocks"""
    if a.dtype != torch.float32:
        return a @ b.t()
    block = max(1, block * _ORDER[0] // 16)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in range(0, a.shape[1], block):
        acc = (acc.double() + a[:, k:k + block].double() @ b[:, k:k + block].double().t()).float()
    return acc


class _Lin(torch.autograd.Function):
    """z = a W^T.  Forward: the fp16 operand and the fp16 weights.  Backward: d a = dz bf16(W), d W = dz^T (bf16 image of a); dz
    arrives rounded from the epilogue behind this layer (_Relu, _Gate, _GradRound, _Scale)."""

    @staticmethod
    def forward(ctx, a, a_img, w, rounded):
        ctx.save_for_backward(a_img, w)
        ctx.rounded = rounded
        return _mm(a, _rnd(w, torch.float16) if rounded else w, 16)

    @staticmethod
    def backward(ctx, gz):
        a_img, w = ctx.saved_tensors
        # dgrad: sum over the outputs in k-blocks of 16; wgrad: sum over the samples in wave tiles of 32
        return _mm(gz, (_rnd(w, torch.bfloat16) if ctx.rounded else w).t(), 16), None, _mm(gz.t(), a_img.t(), 32), None


class _Bias(torch.autograd.Function):
    """z + b; backward: d b = the sum of dz over the samples, in _mm's order (the weight-gradient kernel's column of ones)"""

    @staticmethod
    def forward(ctx, z, b):
        return z + b

    @staticmethod
    def backward(ctx, g):
        return g, _mm(g.t(), torch.ones(1, g.shape[0], dtype=g.dtype), 32).reshape(-1)


class _Relu(torch.autograd.Function):
    """relu of the fp32 accumulator; backward: the gradient where acc > 0, rounded to bf16"""

    @staticmethod
    def forward(ctx, z, rounded):
        ctx.save_for_backward(z > 0)
        ctx.rounded = rounded
        return torch.relu(z)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        g = g * mask
        return (_rnd(g, torch.bfloat16) if ctx.rounded else g), None


class _Gate(torch.autograd.Function):
    """s = sigmoid(z); backward: g s (1 - s) with the stashed bf16 gate, rounded to bf16.  drop: the factor is lost (mutation)"""

    @staticmethod
    def forward(ctx, z, rounded, drop):
        s = torch.sigmoid(z)
        ctx.save_for_backward(_rnd(s, torch.bfloat16) if rounded else s)
        ctx.rounded, ctx.drop = rounded, drop
        return s

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        g = g if ctx.drop else g * (s * (1.0 - s))
        return (_rnd(g, torch.bfloat16) if ctx.rounded else g), None, None


class _GradRound(torch.autograd.Function):
    """identity; backward: the summed gradient rounded to bf16 (the small operands, d h)"""

    @staticmethod
    def forward(ctx, x, rounded):
        ctx.rounded = rounded
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (_rnd(g, torch.bfloat16) if ctx.rounded else g), None


class _Blend(torch.autograd.Function):
    """df = sum_k w_k f_k; backward d f_k = w_k d df, or with grids 0 and 2 exchanged (mutation, backward only)"""

    @staticmethod
    def forward(ctx, f0, f1, f2, w, swap):
        ctx.save_for_backward(w)
        ctx.swap = swap
        return w[:, 0:1] * f0 + w[:, 1:2] * f1 + w[:, 2:3] * f2

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        k = (2, 1, 0) if ctx.swap else (0, 1, 2)
        return g * w[:, k[0]:k[0] + 1], g * w[:, k[1]:k[1] + 1], g * w[:, k[2]:k[2] + 1], None, None


class _Scale(torch.autograd.Function):
    """dx = raw * scale; backward: d raw = bf16(fl32(d_dx * scale)), d scale = sum d_dx raw (the fp32 raw, unrounded)"""

    @staticmethod
    def forward(ctx, raw, scale, rounded):
        ctx.save_for_backward(raw, scale)
        ctx.rounded = rounded
        return raw * scale

    @staticmethod
    def backward(ctx, g):
        raw, scale = ctx.saved_tensors
        if ctx.rounded:
            g_raw = (g.float() * scale.float()).to(torch.bfloat16).to(g.dtype)
        else:
            g_raw = g * scale
        return g_raw, _mm((g * raw).reshape(1, -1), torch.ones(1, g.numel(), dtype=g.dtype), 96).reshape(scale.shape), None


def _layer(a, a_img, w, rounded, trace, name):
    """_Lin, and for the screens of select_rows: (name, z, the operand, the weights) of a layer whose output enters a ReLU"""
    z = _Lin.apply(a, a_img, w, rounded)
    if trace is not None:
        trace.append((name, z.detach(), a.detach(), (_rnd(w, torch.float16) if rounded else w.detach())))
    return z


def fourier(x, n_freq, dtype, shift_column=None):
    """[x | sin(a_0) | cos(a_0) | sin(a_1) | ...] for x [n,d] fp32, with the reference's fp32 argument a_b = fl(fl(x 2^b) pi_f32)
    (src/embeddings.py:28-32; what csrc/mlp_chain.h::sincos_rev reproduces) and the sine / cosine of that argument taken in
    float64.  shift_column: that column's band is one too high (mutation)."""
    x = x.detach().float()
    cols = [x.double()]
    for b in range(n_freq):
        for k, fn in enumerate((torch.sin, torch.cos)):
            first = x.shape[1] * (1 + 2 * b + k)
            parts = []
            for c in range(x.shape[1]):
                band = b + 1 if shift_column == first + c else b
                arg = (x[:, c] * float(2.0 ** band)) * torch.tensor(math.pi, dtype=torch.float32)
                parts.append(fn(arg.double()))
            cols.append(torch.stack(parts, -1))
    return torch.cat(cols, -1).to(dtype)


def triangle_weights(t):
    """p4mlp.hip::triangle_weights in fp32: clamp(1 - |t - a| / 0.5, 0, 1) around a = 0, 0.5, 1, divided by 1e-8f + their sum
    added in the order 0, 0.5, 1 (reference src/core.py:324-332).  t [n] fp32 -> [n,3] fp32"""
    t = t.detach().float().reshape(-1)
    w = [torch.clamp(1.0 - torch.abs(t - a) / 0.5, 0.0, 1.0) for a in (0.0, 0.5, 1.0)]
    s = torch.full_like(t, 1e-8)
    for k in range(3):
        s = s + w[k]
    return torch.stack([w[k] / s for k in range(3)], -1)


def blocks_of(flat, dtype):
    """{name: live slice of the block as a differentiable view of flat}"""
    flat = flat.to(dtype)
    return {name: flat[off:off + int(np.prod(shape))].view(shape)[tuple(slice(0, v) for v in live)] for name, off, shape, live in BLOCKS}


def deform_chain(flat, feats, t, x, blend=None, rounded=True, dtype=torch.float64, mutate=None, trace=None):
    """(dx [n,3], x_c [n,3]) of the deformation chain.  flat: the parameter vector (a leaf for gradients); feats: three [n,24]
    tensors (fp32 hash features; rounded to fp16 here when ``rounded``; leaves for d_feat); t [n] fp32; x [n,3]; blend [n,3] or None"""
    assert mutate in MUTATIONS
    P = blocks_of(flat, dtype)
    r = rounded
    op = lambda v: _st(v, torch.float16, r)
    tc = fourier(t.reshape(-1, 1), 10, dtype, SHIFTED_TIME_COLUMN if mutate == "shift_time_band" else None)
    tc1 = torch.cat([tc, torch.ones_like(tc[:, :1])], -1)
    h1 = _Relu.apply(_layer(op(tc1), _img(tc1, r), torch.cat([P["T1W"], P["T1b"][:, None]], 1), r, trace, "T1"), r)
    tm = _Gate.apply(_Bias.apply(_Lin.apply(op(h1), _img(h1, r), P["T2W"], r), P["T2b"]), r, mutate == "drop_gate_derivative")
    w = (triangle_weights(t) if blend is None else blend.detach().float()).to(dtype)
    f = [op(v.to(dtype)) for v in feats]
    df = _Blend.apply(f[0], f[1], f[2], w, mutate == "swap_blend_weights")
    cat = torch.cat([df, tm], -1)
    hd1 = _Relu.apply(_layer(op(cat), _img(cat, r), P["D1"], r, trace, "D1"), r)
    hd2 = _Relu.apply(_layer(op(hd1), _img(hd1, r), P["D2"], r, trace, "D2"), r)
    raw = _Lin.apply(op(hd2), _img(hd2, r), P["D3"], r)
    dx = _Scale.apply(raw, P["scale"], r)
    return dx, x.to(dtype) + dx


def canon_chain(flat, feat, t, dirs, rounded=True, dtype=torch.float64, mutate=None, trace=None):
    """(rgb [n,3], sigma [n]) of the canonical chain on feat [n,32] (fp32 hash features; a leaf for d_feat), t [n], unit dirs [n,3]"""
    assert mutate in MUTATIONS
    P = blocks_of(flat, dtype)
    r = rounded
    op = lambda v: _st(v, torch.float16, r)
    tc = fourier(t.reshape(-1, 1), 10, dtype, SHIFTED_TIME_COLUMN if mutate == "shift_time_band" else None)
    denc = fourier(dirs, 4, dtype)
    f16 = op(feat.to(dtype))
    xin = torch.cat([f16, op(tc)], -1)
    ximg = torch.cat([_img(f16, r), _img(tc, r)], -1)             # bf16 of the fp16 image; bf16 of the fp32 code
    hs1 = _Relu.apply(_layer(xin, ximg, P["S1"], r, trace, "S1"), r)
    h = _GradRound.apply(_Lin.apply(op(hs1), _img(hs1, r), P["S2"], r), r)
    sigma = torch.nn.functional.softplus(h[:, 0] - 5.0)
    cin = torch.cat([h, denc], -1)
    hc1 = _Relu.apply(_layer(op(cin), _img(cin, r), P["C1"], r, trace, "C1"), r)
    hc2 = _Relu.apply(_layer(op(hc1), _img(hc1, r), P["C2"], r, trace, "C2"), r)
    rgb = torch.sigmoid(_GradRound.apply(_Lin.apply(op(hc2), _img(hc2, r), P["C3"], r), r))
    return rgb, sigma


def evaluate(flat, feats, feat_c, t, dirs, x, blend, d_dx, d_rgb, d_sigma, rounded=True, dtype=torch.float64, mutate=None):
    """Both chains, each on the features handed to it (the canonical chain is NOT fed the deformation chain's x_c), and their
    backward from the upstream gradients.  Returns a dict: dx, x_c, rgb, sigma, grads (flat [30145]; pads zero), d_feat (four tensors)."""
    flat = flat.detach().to(dtype).requires_grad_(True)
    leaves = [v.detach().to(dtype).requires_grad_(True) for v in list(feats) + [feat_c]]
    with torch.enable_grad():
        dx, xc = deform_chain(flat, leaves[:3], t, x, blend, rounded, dtype, mutate)
        rgb, sigma = canon_chain(flat, leaves[3], t, dirs, rounded, dtype, mutate)
        loss = (dx * d_dx.to(dtype)).sum() + (rgb * d_rgb.to(dtype)).sum() + (sigma * d_sigma.to(dtype)).sum()
        g = torch.autograd.grad(loss, [flat] + leaves)
    return dict(dx=dx.detach(), x_c=xc.detach(), rgb=rgb.detach(), sigma=sigma.detach(), grads=g[0], d_feat=list(g[1:]))


# ------------------------------------------------------------------------------------------------------------------ quantities
def live(grads, name):
    """the live slice of block ``name`` of a flat gradient vector"""
    _, off, shape, lv = next(b for b in BLOCKS if b[0] == name)
    return grads[off:off + int(np.prod(shape))].view(shape)[tuple(slice(0, v) for v in lv)]


def pad_mask():
    """bool [30145]: the entries of the flat vector that no chain reads (pad rows and columns)"""
    m = torch.ones(N_PARAMS, dtype=torch.bool)
    for name, off, shape, lv in BLOCKS:
        blk = torch.ones(shape, dtype=torch.bool)
        blk[tuple(slice(0, v) for v in lv)] = False
        m[off:off + int(np.prod(shape))] = blk.reshape(-1)
    return m


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def figures(got, ref, chains=("deform", "canon")):
    """{quantity: (figure, kind)} of ``got`` against ``ref`` (both dicts as evaluate returns them): the quantities the bounds are
    formed for.  kind: 'fwd' (fp16-rounded forward output), 'grad' (bf16-rounded), 'fp32' (summed in fp32 only)."""
    out = {}
    if "deform" in chains:
        out["dx"] = (float((got["dx"].double().cpu() - ref["dx"].double().cpu()).abs().max() / ref["dx"].double().abs().max()), "fwd")
    if "canon" in chains:
        out["rgb"] = (float((got["rgb"].double().cpu() - ref["rgb"].double().cpu()).abs().max()), "fwd")
        out["sigma"] = (rel_l2(got["sigma"].reshape(-1), ref["sigma"].reshape(-1)), "fwd")
    names = (DEFORM_BLOCKS if "deform" in chains else ()) + (CANON_BLOCKS if "canon" in chains else ())
    for name in names:
        out[name] = (rel_l2(live(got["grads"], name), live(ref["grads"], name)), "fp32" if name == "scale" else "grad")
    for blk, name, c0, c1 in INPUT_BLOCKS:
        if blk in names:
            out[name] = (rel_l2(live(got["grads"], blk)[:, c0:c1], live(ref["grads"], blk)[:, c0:c1]), "grad")
    for k in range(4):
        if ("deform" in chains and k < 3) or ("canon" in chains and k == 3):
            out[f"d_feat[{k}]"] = (rel_l2(got["d_feat"][k], ref["d_feat"][k]), "fp32")
    return out


def bound_of(yard, kind):
    """max(floor, 4 x yardstick); the caps are asserted on 4 x yardstick by tests/test_part4_reference.py"""
    return max({"fwd": FLOOR_FP16, "grad": FLOOR_BF16, "fp32": FLOOR_FP32}[kind], 4.0 * yard)


# ------------------------------------------------------------------------------------------------------------------ inputs
def golden_flat(g):
    """the flat parameter vector from a golden's ``w:`` entries (project-nerf_amd/part4.py::MODULE_SLICES order)"""
    keys = ("time_modulation.net.0.weight", "time_modulation.net.0.bias", "time_modulation.net.2.weight", "time_modulation.net.2.bias",
            "deform_decoder.deform_net.params", "decoder.sigma_net.params", "decoder.color_net.params", "deform_decoder.displacement_scale")
    flat = torch.cat([torch.from_numpy(np.asarray(g["w:" + k])).reshape(-1).float() for k in keys])
    assert flat.numel() == N_PARAMS
    return flat


N_CANDIDATES, PLANT_TRIES = 8192, 64
_HALF = np.float32(0.5)
PLANTED_T = (0.0, 0.5, 1.0, float(np.nextafter(_HALF, np.float32(0))), float(np.nextafter(_HALF, np.float32(1))), 0.25)
CODE_TIE_EPS = 2.0 ** -20        # the hardware sine (v_sin_f32, no quotable bound) was seen to move ~2e-7: five times that
MASK_MARGIN_UNITS = 4.0          # a ReLU input stays this many fp16 units of its largest term away from zero


def tie_distance(v, mantissa):
    """distance of the float64 values v from the nearest rounding tie of a format with ``mantissa`` stored bits (normal range)"""
    spacing = torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-30))) - mantissa)
    nearest = torch.round(v / spacing) * spacing
    return spacing / 2 - (v - nearest).abs()


def code_rows_ok(x, n_freq):
    """rows of x [m,d] whose Fourier code is DEFINED by the rounding points: no sine or cosine of magnitude >= 2^-9 within CODE_TIE_EPS
    of an fp16 or bf16 rounding tie.  The kernels take them from the hardware sine; where the exact value sits closer to a tie than
    that instruction's error, which 16-bit value the chain sees is the instruction's choice, not the restatement's."""
    v = fourier(x, n_freq, torch.float64)[:, x.shape[1]:]
    near = (tie_distance(v, 10) < CODE_TIE_EPS) | (tie_distance(v, 7) < CODE_TIE_EPS)
    return ~((v.abs() >= 2.0 ** -9) & near).any(-1)


def mask_rows_ok(flat, feats, t, dirs, x, blend):
    """rows whose every ReLU input, in the matched float64 chain, is further from zero than MASK_MARGIN_UNITS fp16 units of the largest
    term of its sum.  One operand landing on the other fp16 neighbour (another summation order, the hardware sine or exponential)
    moves the sum by one such unit; where that can change the sign, the ReLU's bit -- and with it the sample's whole gradient behind
    that unit -- is decided by the order of a sum: one such row among 127 moved every canonical gradient by 0.5-1 %."""
    ok = torch.ones(t.shape[0], dtype=torch.bool)
    for a in range(0, t.shape[0], 512):
        rows = slice(a, a + 512)
        trace = []
        with torch.no_grad():
            for bl in (None, blend[rows]):
                deform_chain(flat, [f[rows] for f in feats[:3]], t[rows], x[rows], bl, True, torch.float64, None, trace)
            canon_chain(flat, feats[3][rows], t[rows], dirs[rows], True, torch.float64, None, trace)
        for name, z, op, w in trace:
            if name in ("T1", "S1"):       # their operands are the hash image and the codes: exact, or held off the ties by code_rows_ok
                continue
            unit = 2.0 ** -10 * (op.abs()[:, None, :] * w.abs()[None]).amax(-1)
            ok[rows] &= (z.abs() >= MASK_MARGIN_UNITS * unit).all(-1)
    return ok


def _pool(golden):
    """the candidate draw, both parameter sets, and the rows select_rows keeps; made once"""
    if "pool" in _YARD:
        return _YARD["pool"]
    g = torch.Generator().manual_seed(4105)
    m = N_CANDIDATES
    c = {}
    c["pts"] = (torch.rand(m, 3, generator=g) - 0.5) * 2 * BOUND * 0.98          # the deformation grids' query points = x
    c["pts_c"] = (torch.rand(m, 3, generator=g) - 0.5) * 2 * BOUND * 0.98        # the canonical grid's: arbitrary points
    c["dirs"] = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=-1)
    c["t"] = torch.rand(m, generator=g)
    for j, v in enumerate(PLANTED_T):                                              # PLANT_TRIES candidate rows per planted time
        c["t"][j * PLANT_TRIES:(j + 1) * PLANT_TRIES] = v
    c["d_dx"] = torch.randn(m, 3, generator=g) * 0.5 + 0.3
    c["d_rgb"] = torch.randn(m, 3, generator=g) * 0.5 + 0.3
    c["d_sigma"] = torch.randn(m, generator=g) * 0.5 + 0.3
    c["blend"] = torch.rand(m, 3, generator=g) * 0.9 + torch.tensor([0.2, 1.3, 2.4])      # not normalised, pairwise distinct
    c["levels_d"], c["levels_c"] = O.hash_grid_levels(*LEVELS_D), O.hash_grid_levels(*LEVELS_C)
    c["tables"] = [(torch.rand(O.hash_grid_entries(lv), 2, generator=g) - 0.5).contiguous()
                   for lv in (c["levels_d"], c["levels_d"], c["levels_d"], c["levels_c"])]
    flats = {"golden": golden_flat(golden), "random": (torch.rand(N_PARAMS, generator=g) * 2 - 1) * 0.3}
    flats["random"][D3:S1] = flats["random"][D3:S1].abs()      # one sign in the displacement head (cancellation: chain_inputs)
    for f in flats.values():
        f[SCALE] = 0.1
    feats = cpu_features(c)
    planted = torch.arange(m) < len(PLANTED_T) * PLANT_TRIES
    ok = code_rows_ok(c["dirs"], 4) & code_rows_ok(c["t"].reshape(-1, 1), 10)
    for f in flats.values():
        ok &= mask_rows_ok(f, feats, c["t"], c["dirs"], c["pts"], c["blend"])
    rows = []
    for j in range(len(PLANTED_T)):
        block = torch.nonzero(ok[j * PLANT_TRIES:(j + 1) * PLANT_TRIES]).reshape(-1)
        assert block.numel() > 0, f"no candidate row passes the screens at planted t = {PLANTED_T[j]}"
        rows.append(int(block[0]) + j * PLANT_TRIES)
    rest = torch.nonzero(ok & ~planted).reshape(-1)
    assert rest.numel() >= N_POOL - len(rows), f"only {rest.numel()} of {m} candidate rows pass the screens"
    rows = torch.tensor(rows + rest[:N_POOL - len(rows)].tolist())
    _YARD["pool"] = (c, flats, rows, float(ok.float().mean()))
    return _YARD["pool"]


def chain_inputs(which, golden):
    """The GPU tests' inputs, made on the CPU (tests/test_gpu_part4_chains.py moves them over; tests/test_part4_reference.py measures
    the yardsticks on them): 1,025 rows of one fixed draw, a case uses the first n.  which: 'golden' (g14's network weights) or
    'random' (one draw over the whole flat vector, pads filled too; the three live rows of D3 made one-signed: with zero-mean rows dx
    is a difference of terms larger than itself, and one fp16 unit of one activation -- what any fp16 chain may differ by -- came
    to 5.2e-4 .. 5.6e-4 of max |dx|, four times which is over the 2e-3 cap).  displacement_scale 0.1; upstream gradients with a
    non-zero mean (tests/test_gpu_wgrad_sums.py's docstring); t in [0,1] with 0, 0.5, 1, the two fp32 neighbours of 0.5 and 0.25 in
    the first six rows.  The rows are the first of N_CANDIDATES drawn that pass two screens, both computed from the restatement alone,
    for both parameter sets (code_rows_ok, mask_rows_ok): rows on which the matched answer is defined by the rounding points."""
    c, flats, rows, _ = _pool(golden)
    out = {k: (v[rows].contiguous() if isinstance(v, torch.Tensor) and v.shape[0] == N_CANDIDATES else v) for k, v in c.items()}
    out["which"], out["flat"] = which, flats[which].clone().contiguous()
    return out


def cpu_features(c):
    """fp32 hash features of the inputs from the oracle's hash grid: [three [n,24], one [n,32]]"""
    x01, x01c = O.hash_normalise(c["pts"], BOUND), O.hash_normalise(c["pts_c"], BOUND)
    return [O.hash_encode(c["levels_d"], c["tables"][k], x01) for k in range(3)] + [O.hash_encode(c["levels_c"], c["tables"][3], x01c)]


def evaluate_inputs(c, feats, n, blend=False, **kw):
    """evaluate() on the first n rows of chain_inputs' draw with the given features (four tensors of at least n rows)"""
    return evaluate(c["flat"], [f[:n] for f in feats[:3]], feats[3][:n], c["t"][:n], c["dirs"][:n], c["pts"][:n],
                    c["blend"][:n] if blend else None, c["d_dx"][:n], c["d_rgb"][:n], c["d_sigma"][:n], **kw)


YARD_CASES = tuple((which, n, blend) for which in ("golden", "random") for n in SWEEP for blend in (False, True) if not blend or n in (129, 1025))
_YARD = {}


def yardstick_case(which, n, blend, golden):
    """({quantity: (figure, kind)}, the float64 side) of one case: the matched chain with float32 sums against itself with float64
    sums, on chain_inputs with the oracle's features; computed once per case"""
    key = (which, n, blend)
    if key not in _YARD:
        if ("inputs", which) not in _YARD:
            c = chain_inputs(which, golden)
            _YARD[("inputs", which)] = (c, cpu_features(c))
        c, feats = _YARD[("inputs", which)]
        r64 = evaluate_inputs(c, feats, n, blend, rounded=True, dtype=torch.float64)
        fig = {}
        for order in ORDERS:                     # several float32 orders: which one meets a rounding boundary is chance
            _ORDER[0] = order
            try:
                f32 = figures(evaluate_inputs(c, feats, n, blend, rounded=True, dtype=torch.float32), r64)
            finally:
                _ORDER[0] = ORDERS[0]
            fig = {k: (max(v[0], fig.get(k, (0.0,))[0]), v[1]) for k, v in f32.items()}
        _YARD[key] = (fig, r64)
    return _YARD[key]


def yardsticks(golden):
    """{quantity: (yardstick, kind)}: per quantity, the LARGEST figure over YARD_CASES (every case of the GPU sweep, both parameter
    sets, blend None and explicit).  Pooled because what the figure measures is an event -- a sum that lands on the other side of a
    16-bit rounding boundary in the other summation order -- whose rate belongs to the inputs, while which case catches one is chance:
    most cases see none (figures of 1e-7), a few see one, and the GPU's own order meets others at other samples.  For the same reason
    the float32 side is evaluated in every order of ORDERS (yardstick_case): with one order alone the pooled figure of a quantity is
    one event's or none's."""
    out = {}
    for which, n, blend in YARD_CASES:
        for name, (fig, kind) in yardstick_case(which, n, blend, golden)[0].items():
            if fig >= out.get(name, (-1.0, kind))[0]:
                out[name] = (fig, kind)
    return out


def bounds(golden):
    """{quantity: max(floor, 4 x yardstick)}: the bounds tests/test_gpu_part4_chains.py holds the kernels to"""
    return {name: bound_of(fig, kind) for name, (fig, kind) in yardsticks(golden).items()}
